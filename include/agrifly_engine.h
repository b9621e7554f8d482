/*
 * agrifly_engine.h -- C ABI of the MI355X batched quadrotor dynamics engine.
 *
 * This is the drop-in boundary for agri-fly's vehicle-step hot path.  The
 * reference has no FFI: its seams are a C++ abstract class and a template
 * parameter compiled in-process.  The entry points below are
 * what a binding of that path has to reach; each one names the reference
 * interface it replaces (paths relative to the agri-fly tree).  The C++ facade
 * in include/agrifly/ re-creates the reference's Vehicle / logicType classes
 * on top of exactly these calls.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ or torch types.
 *   - every call returns an afe_status (0 = ok); no exceptions cross the ABI;
 *     afe_last_error() gives the message of the last failure on that engine.
 *   - host arrays are caller-allocated and PLANAR: a 3-vector field of `count`
 *     vehicles is x[0..count) y[0..count) z[0..count); quaternions are scalar
 *     first (w x y z), as Common/Common/Math/Rotation.hpp:46-51.
 *   - one engine = one ensemble on one GPU with one clock; one host thread at
 *     a time per engine (the reference is single-threaded as well).
 *   - stepping is asynchronous on the engine's HIP stream; getters synchronise.
 *   - there is NO CPU fallback: without a usable gfx950 device afe_create
 *     fails with AFE_ERR_NO_DEVICE.
 */
#ifndef AGRIFLY_ENGINE_H
#define AGRIFLY_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: afe_device_view starts with `struct_bytes` (set by the caller; the engine never writes past it) and carries
 *    pos_anchor_xy -- AFE_F32 engines keep x and y in `pos` RELATIVE to the last set point (round 3 changed the meaning of
 *    view.pos without changing this number: a host built against version 1 must be rebuilt, afe_abi_version() tells). */
/* 3: afe_set_reserved_compute_units is gone (no consumer; a reservation cost the grid 4-25 %); added
 *    afe_has_dev_hooks and afe_persistent_kernarg_layout.  Nothing else moved: a version-2 host that never called the
 *    removed function runs unchanged after a rebuild. */
#define AFE_ABI_VERSION 3

typedef struct afe_engine afe_engine; /* opaque */

typedef enum afe_status {
  AFE_OK = 0,
  AFE_ERR_INVALID_ARG = 1,
  AFE_ERR_NO_DEVICE = 2,   /* no HIP device / not gfx950 / kernels missing */
  AFE_ERR_HIP = 3,         /* a HIP runtime call failed (see afe_last_error) */
  AFE_ERR_OUT_OF_RANGE = 4,
  AFE_ERR_NOT_CONFIGURED = 5, /* stepping before a type table was set */
  AFE_ERR_COMM = 6
} afe_status;

typedef enum afe_precision {
  AFE_F32 = 0, /* fp32 state + arithmetic: the production path (176 B/step) */
  AFE_F64 = 1  /* fp64 state + arithmetic: the reference's own precision */
} afe_precision;

typedef enum afe_seed_policy {
  /* every vehicle seeds std::default_random_engine with 1, exactly like the
   * reference ensemble does (Quadcopter_T.cpp:27) */
  AFE_SEED_REFERENCE = 0,
  /* seed = 1 + global vehicle index: independent Monte-Carlo streams */
  AFE_SEED_DECORRELATED = 1,
  /* Monte-Carlo ensembles that need no libstdc++ stream: the six normals of (vehicle, logic tick) come from a
   * counter-based generator -- Philox4x32-10 keyed by afe_set_noise_seed, addressed by the GLOBAL vehicle index and
   * the tick number, Box-Muller on top:
   *   key = (seed low, seed high); counter = (index low, index high (16 bits) | stream << 16 | block << 24, ordinal low,
   *   ordinal high); stream 1 = IMU noise (ordinal = logic-tick number; blocks 0 and 1 give z0..z7: gyro x y z = z0 z1 z2,
   *   accelerometer x y z = z3 z4 z5), stream 2 = gusts (ordinal = epoch; block 0: force = sigma_i (z0, z1, z2));
   *   per pair of words: u_r = ((x_even >> 9) + 0.5) 2^-23, u_a = (x_odd >> 8) 2^-24 (both exact in fp32),
   *   r = sqrt(-2 ln u_r), z_a = r cos(2 pi u_a), z_b = r sin(2 pi u_a)   (|z| <= 5.65).
   * The AFE_F64 engine evaluates this in double (1e-13 of a libm evaluation), the AFE_F32 engine in float with the
   * hardware reciprocal / square root / sine / cosine (measured worst 6e-7 absolute).  No per-vehicle engine word
   * is loaded or stored, nothing diverges (no rejection loop); the samples do not depend on how the ensemble is
   * sharded, stepped or fused.  The reference produces no such stream (it seeds every vehicle with 1). */
  AFE_SEED_COUNTER = 2
} afe_seed_policy;

/* The per-vehicle constant record: the arguments of
 *   Simulation::Quadcopter_T<logicType>::Quadcopter_T(...)
 *   Components/Components/Simulation/Quadcopter_T.hpp:24-32
 * (masterTimer, id and quadcopterType are engine / facade concerns).  The
 * engine derives motor geometry, I^-1 and the IMU mount matrix from it the way
 * the ctor body does (Quadcopter_T.cpp:20,45-65,75-80). */
typedef struct afe_vehicle_params {
  double mass;                       /* [kg] */
  double inertia[9];                 /* row-major 3x3 [kg m^2] */
  double arm_length;                 /* [m] */
  double com_error[3];               /* centreOfMassError [m] */
  double motor_min_speed;            /* [rad/s] */
  double motor_max_speed;            /* [rad/s] */
  double prop_thrust_from_speed_sqr; /* [N/(rad/s)^2] */
  double prop_torque_from_speed_sqr; /* [N m/(rad/s)^2] */
  double motor_time_const;           /* [s]; 0 = instantaneous */
  double motor_inertia;              /* [kg m^2] */
  double lin_drag_coeff_b[3];        /* [N s/m], body axes */
  float imu_yaw, imu_pitch, imu_roll; /* QuadcopterConstants::IMU_* [rad] */
} afe_vehicle_params;

/* ---- vehicle-type table -------------------------------------------------
 * Replaces Onboard::QuadcopterConstants(QuadcopterType) +
 * GetVehicleTypeFromID (Components/Components/Logic/QuadcopterConstants.hpp:
 * 31-274,297-332) as consumed by Simulator/Rappids_Simulator/main.cpp:147-218.
 * type: 1 CF_STANDARD, 2 CF_BIGMOTORSPROPS, 4 CF_LARGEQUAD, 5 CF_MINIQUAD.
 * Pure host functions: usable without a GPU. */
int afe_params_from_type(int quadcopter_type, afe_vehicle_params *out);
int afe_type_from_id(unsigned vehicle_id);
/* QuadcopterConstants(type).lowBatteryThreshold [V] for every type 0..5, the refused ones included -- perCellLowVoltage
 * 3 V (QuadcopterConstants.hpp:50-51) times the cell count: 0 INVALID (:51), 1 CF_STANDARD 3 V (:83),
 * 2 CF_BIGMOTORSPROPS 3 V (:117), 3 CF_FEEDTHROUGH 3 V (:150), 4 CF_LARGEQUAD 9 V (:180), 5 CF_MINIQUAD 6 V (:220).  The
 * reference's vehicle hands its logic 1.2 x this as the battery measurement at every tick (Quadcopter_T.cpp:72, 163).
 * NULL output or a type outside 0..5: AFE_ERR_INVALID_ARG. */
int afe_low_battery_threshold_from_type(int quadcopter_type, float *volts);

/* ---- lifetime -----------------------------------------------------------
 * Replaces `new Simulation::Quadcopter(...)` x n_vehicles (main.cpp:211-218;
 * the multi-vehicle form is the std::vector<SimVehicle> of
 * AIFS_ROS/hiperlab_rostools/src/Simulator/main.cpp:58-95).
 * device < 0 selects the current HIP device.  first_global_index is this
 * shard's offset in the whole ensemble (used by AFE_SEED_DECORRELATED and by
 * afe_nearest_neighbour's self-exclusion); 0 for a single-GPU ensemble.  Initial state is the
 * reference's: origin, at rest, identity attitude, motors stopped, engine
 * clock 0 (SimulationObject6DOF.hpp:14-19, Motor.cpp:18). */
int afe_create(afe_engine **out, int64_t n_vehicles, int precision, int device,
               int64_t first_global_index);
/* The same engine with its state arena in pinned, coherent HOST memory that the device addresses over the bus -- for
 * small ensembles with the host in the loop of every step (one `Quadcopter_T::Run()` + `GetPosition()` per millisecond,
 * Simulator/Rappids_Simulator/main.cpp:330-392; the onboard logic of Quadcopter_T.cpp:159-189 on the host).  Getters
 * and setters of state, commands, wrench and IMU are then plain copies inside host memory once the steps authorised so
 * far are done: no transfer call, and a resident grid (the engine starts in AFE_STEP_AUTO) is NOT parked by them.
 * One step of that loop then costs ~9 us instead of ~75 (one vehicle, MI355X).  A step's loads and stores cross the bus
 * (~1.5 us of latency, all in flight together), so this is the wrong
 * choice for ensembles that step many times between host visits or hold more than a few thousand vehicles.
 * Same results, bit for bit, as afe_create; every other entry point behaves the same. */
int afe_create_host_visible(afe_engine **out, int64_t n_vehicles, int precision, int device,
                            int64_t first_global_index);
int afe_destroy(afe_engine *e);
const char *afe_last_error(const afe_engine *e);
const char *afe_status_string(int status);
int afe_abi_version(void);
/* 1 when the loaded library was built with -DAFE_DEV_HOOKS (the kernel lab's measurement variables of tools/ are
 * read), 0 for the release build, which reads exactly six environment variables:
 * AFE_PERSIST_AQL, AFE_FORCE_STEP_MODE, AFE_FORCE_SPLIT, AFE_FORCE_HOST_ARENA, AFE_PERSIST_DEBUG, AFE_GRID_LOG. */
int afe_has_dev_hooks(void);
/* Build self-check (no GPU needed): byte offset and size of each of the four by-value arguments of the resident step
 * kernel -- StepView, DevParams, DevLogic, PersistArgs -- as the HOST packs them for a dispatch on the engine's own
 * queue (precision AFE_F32 / AFE_F64), and the size of the whole segment.  tests/test_kernel_resources.py holds them
 * against the argument table of every instantiation in the gfx950 code object inside the library. */
int afe_persistent_kernarg_layout(int precision, int32_t offsets[4], int32_t sizes[4], int32_t *segment_bytes);

/* Use a caller-owned HIP stream (hipStream_t) for all engine work, e.g. a torch.cuda.Stream()'s .cuda_stream, so that
 * the engine's work is part of the host's own stream and needs no synchronisation against it.
 *   What is ordered.  From the return of this call every entry point that takes the engine queues on that stream, in
 *     call order, with whatever the host queues there itself: afe_step's launches, the setters' and getters' copies,
 *     afe_pack_positions, afe_gather_positions, afe_event_record, the neighbour queries, afe_uwb_range, and the
 *     library's consumers of the engine's state -- depth camera (afe_render_depth_engine), clearance query and plan
 *     audits (afe_clearance_*_engine*), contact monitor, statistics -- which fetch the stream at every call.  Work the
 *     host queued before an engine call is seen by it (a buffer filled on the stream and queried at once); work the host
 *     queues after afe_step has returned sees the stepped slabs (afe_get_device_view): order at return.
 *     afe_nearest_neighbour_async runs on a stream of the engine's own that is ordered behind the caller's stream at
 *     the call; its results are the host's after afe_query_sync, as on the engine's own stream.
 *   The exception.  afe_set_split_stepping(e, 2) keeps half of every step on a second stream of the engine's: the
 *     caller's stream is then ordered behind the steps only at the NEXT engine call that touches device state or the
 *     stream (see there) -- put afe_event_record or afe_sync between afe_step and the host's own reader.  The automatic
 *     split (parts = 0) never engages on a caller's stream, nor do the resident grid and the engine's own queue: on a
 *     caller's stream afe_step is the launches, whatever step mode is set (afe_persistent_running stays 0).  Same bits.
 *   Not engine-bound.  Entry points that take a device, a scene or a map, not an engine -- afe_rappids_plan*,
 *     afe_image_truth_*, afe_render_depth, afe_clearance_query / _segments / _paths*, afe_device_upload / _download --
 *     are NOT moved by this call: they run on the device's default (NULL) stream, which does not wait for non-blocking
 *     streams such as torch's.  A host that produced device input for one of them (afe_rappids_plan_device's images,
 *     afe_image_truth_*'s with images_on_device, afe_device_download's source) on a stream of its own synchronises that
 *     stream (hipStreamSynchronize, or an event) before the call; their results are complete at return.
 *   Handle 0.  NULL restores the engine's own stream -- it does NOT mean the default stream, although the default
 *     stream's handle is 0 (torch.cuda.default_stream().cuda_stream == 0): work a host queues on the default stream is
 *     not ordered against an engine that was given 0.  The default stream is NOT SUPPORTED as a caller's stream: HIP's
 *     reserved handles for it, hipStreamLegacy ((hipStream_t)1) and hipStreamPerThread ((hipStream_t)2), are refused
 *     with AFE_ERR_INVALID_ARG and the engine stays where it was (the engine records events on its stream and makes
 *     its other streams wait for them; the runtime does not take that with a reserved handle).  A host uses a stream
 *     of its own (torch.cuda.Stream()) and queues there what the engine is to be ordered with.
 *   Switching.  The call returns after everything queued on the old stream (a pending half of a split step, a
 *     resident grid's last step) has finished, so nothing of the engine's is left on a stream it has given up.
 *   Lifetime.  The stream stays the caller's: the library never destroys it.  It must outlive the engine, or the
 *     afe_set_stream(e, NULL) (or another stream) that takes the engine off it; afe_destroy waits for it before it frees
 *     the slabs.  NULL engine: AFE_ERR_INVALID_ARG. */
int afe_set_stream(afe_engine *e, void *hip_stream);

/* ---- configuration ------------------------------------------------------ */
/* Table of up to 256 parameter records; vehicle i uses table[type_index[i]].
 * Replaces the per-object ctor args.  How the step kernel gets at a record:
 * all vehicles on record 0 -> kernel arguments; the type index constant over
 * every aligned run of 64 vehicles (a fleet laid out type by type) -> one
 * scalar-loaded record per wave, as fast as the homogeneous case whatever the
 * table size; types mixed within a run of 64 -> the table is staged into LDS
 * per workgroup (slower as the table grows).  Results are the same bits. */
int afe_set_type_table(afe_engine *e, const afe_vehicle_params *table, int n_types);
int afe_set_vehicle_types(afe_engine *e, int64_t first, int64_t count,
                          const uint8_t *type_index);
/* onboardLogicPeriod ctor argument (Quadcopter_T.hpp:32, used at
 * Quadcopter_T.cpp:159-160).  Default 1/500 s (main.cpp:177). */
int afe_set_logic_period(afe_engine *e, double seconds);
/* IMU noise (Quadcopter_T.cpp:5-6,165-180).  The reference hard-codes
 * sigma_gyro = 0.1, sigma_acc = 0.2 and seed 1; these are the defaults.
 * enabled = 0 switches the six draws off (the stream does not advance).
 * The std::minstd_rand0 words and the polar method's accept / reject decisions
 * are libstdc++'s bit for bit in both precisions; the six normal values are
 * libstdc++'s doubles (to 4e-15) in the AFE_F64 engine and float evaluations of
 * the same expression (~4e-7 relative) in the AFE_F32 engine. */
int afe_set_imu_noise(afe_engine *e, int enabled, double sigma_gyro,
                      double sigma_acc, int seed_policy);

/* ---- state in / out -----------------------------------------------------
 * Replace SimulationObject6DOF::Set/Get{Position,Velocity,Attitude,
 * AngularVelocity} (Components/Components/Simulation/SimulationObject6DOF.hpp:
 * 26-56) and Motor::SetSpeed / the motor speed read behind GetMotorForce
 * (Motor.hpp:30-32, Quadcopter_T.hpp:39).  NULL field pointers are skipped. */
int afe_set_state(afe_engine *e, int64_t first, int64_t count,
                  const double *pos3, const double *vel3, const double *att4,
                  const double *ang_vel3, const double *motor_speed4);
int afe_get_state(afe_engine *e, int64_t first, int64_t count, double *pos3,
                  double *vel3, double *att4, double *ang_vel3,
                  double *motor_speed4);
int afe_set_state_f32(afe_engine *e, int64_t first, int64_t count,
                      const float *pos3, const float *vel3, const float *att4,
                      const float *ang_vel3, const float *motor_speed4);
int afe_get_state_f32(afe_engine *e, int64_t first, int64_t count, float *pos3,
                      float *vel3, float *att4, float *ang_vel3,
                      float *motor_speed4);
/* per-vehicle std::minstd_rand0 word (Quadcopter_T.hpp:122); checkpointing */
int afe_set_rng_state(afe_engine *e, int64_t first, int64_t count, const uint32_t *state);
int afe_get_rng_state(afe_engine *e, int64_t first, int64_t count, uint32_t *state);

/* ---- per-tick inputs ----------------------------------------------------
 * afe_set_motor_cmds replaces the read-back of logicType::GetMotorSpeedCmd(i)
 * into _motorSpeedCommands (Quadcopter_T.cpp:187-189; float, Quadcopter_T.hpp:
 * 100).  afe_set_external_force / _torque replace SetExternalForce /
 * SetExternalTorque (Quadcopter_T.hpp:45-51; world frame, persist until
 * replaced).  Passing NULL to the external setters zeroes the range; the
 * kernel only reads the wrench arrays once one has been set non-NULL. */
int afe_set_motor_cmds(afe_engine *e, int64_t first, int64_t count, const float *cmd4);
int afe_set_external_force(afe_engine *e, int64_t first, int64_t count, const double *force3);
int afe_set_external_torque(afe_engine *e, int64_t first, int64_t count, const double *torque3);

/* ---- on-device onboard rates logic (optional) -------
 * Instead of handing each IMU sample to a host-side logicType, the step kernel
 * can run the rates-control slice of Onboard::QuadcopterLogic itself at every
 * logic tick, closing the loop on the GPU:
 *   SetIMUMeasurementRateGyro: _R * gyro -> 2nd-order low-pass
 *       (Components/Components/Logic/QuadcopterLogic.hpp:40-45,
 *        Common/Common/Math/LowPassFilterSecondOrder.hpp:22-64)
 *   KalmanFilter6DOF::Predict without UWB: angular-velocity estimate = filtered
 *       gyro; the first call only initialises (KalmanFilter6DOF.cpp:70-116)
 *   RunControllerExternalRatesControl (QuadcopterLogic.cpp:528-541):
 *       QuadcopterAngularVelocityController::GetDesiredTorques
 *       (QuadcopterAngularVelocityController.hpp:25-38),
 *       QuadcopterMixer::GetMotorForces / PropellerSpeedsFromThrust
 *       (QuadcopterMixer.hpp:63-99)
 * and write the four motor-speed commands, which act from the next step on as
 * in Quadcopter_T.cpp:187-189.  Not included here: the flight-state machine beyond
 * IDLE -> EXTERNAL_RATES_CONTROL, panic checks, attitude estimate, telemetry (the onboard
 * flight computer below, afe_onboard_*, adds them behind the tick), motor calibration
 * (host-side logic).  All logic arithmetic is float, as in
 * the reference.  Record i of the logic table pairs with record i of the
 * vehicle type table. */
typedef struct afe_rates_logic_params {
  float mass;                       /* QuadcopterLogic::_mass */
  float inertia[9];                 /* QuadcopterConstants::inertiaMatrix */
  float ang_vel_time_const_xy;      /* angVelControl_timeConst_xy [s] */
  float ang_vel_time_const_z;       /* angVelControl_timeConst_z [s] */
  float arm_length;                 /* [m] */
  float prop_thrust_from_speed_sqr; /* [N/(rad/s)^2] */
  float prop_torque_from_thrust;    /* [N m/N] */
  int prop0_spin_dir;               /* +1 / -1 */
  float max_thrust_per_propeller;   /* [N] */
  float min_thrust_per_propeller;   /* [N] */
  float max_cmd_total_thrust;       /* [N]; < 0: mixer default 4*max*0.8 */
  float imu_yaw, imu_pitch, imu_roll; /* [rad] */
  float gyro_lowpass_cutoff;        /* [rad/s]; the reference uses 200 */
} afe_rates_logic_params;
/* QuadcopterConstants(type) narrowed to the fields above. Pure host. */
int afe_rates_logic_params_from_type(int quadcopter_type, afe_rates_logic_params *out);
/* Enable (table != NULL) or disable (table == NULL) the on-device logic.
 * Enabling resets the logic state: filters at 0, estimator uninitialised,
 * flight state IDLE (motor commands 0) until afe_set_rates_commands.  The
 * filter sampling period is float(logic period), as Quadcopter_T.cpp:18. */
int afe_set_rates_logic(afe_engine *e, const afe_rates_logic_params *table, int n_types);
/* The decoded externalRatesCmd radio message (RadioTypes.hpp:218-226):
 * floats[0] = total thrust normalised by mass [m/s^2], floats[1..3] = desired
 * body rates [rad/s].  Persists until replaced; puts the vehicles of the range
 * into EXTERNAL_RATES_CONTROL. */
int afe_set_rates_commands(afe_engine *e, int64_t first, int64_t count,
                           const float *thrust_norm, const float *ang_vel3);
/* The command in force (QuadcopterLogic's copy of the last externalRatesCmd, QuadcopterLogic.cpp:293-295): thrust_norm
 * [count], ang_vel3 planar [3][count], have uint8 [count] (1: EXTERNAL_RATES_CONTROL, 0: IDLE).  Any may be NULL,
 * not all. */
int afe_get_rates_commands(afe_engine *e, int64_t first, int64_t count, float *thrust_norm, float *ang_vel3,
                           uint8_t *have);
/* The motor-speed commands currently in force (host- or logic-written). */
int afe_get_motor_cmds(afe_engine *e, int64_t first, int64_t count, float *cmd4);

/* ---- wire formats either side of the step (host-only) --
 * Byte-exact equivalents of RadioTypes::RadioMessageDecoded (Common/Common/
 * DataTypes/RadioTypes.hpp:39-246: 23-byte uplink, type@0 reserved@1 flags@2,
 * ten big-endian 16-bit fixed-point fields) and of TelemetryPacket::
 * Encode/DecodeTelemetryPacket (TelemetryPacket.hpp:32-207: packed
 * {u8 type; u8 packetNumber; u16 data[14]} = 30 bytes).  Usable without a GPU. */
#define AFE_RADIO_PACKET_SIZE 23
#define AFE_TELEMETRY_PACKET_SIZE 30
typedef struct afe_radio_message {  /* RadioMessageDecoded: type, flags, floats[10] */
  uint8_t type;   /* 2 kill, 3 position, 4 acceleration, 5 rates, 6 idle (RadioTypes.hpp:17-25) */
  uint8_t flags;
  float floats[10];
} afe_radio_message;
int afe_radio_create_rates_command(uint8_t flags, float des_total_thrust, const float des_ang_vel[3],
                                   uint8_t raw_out[AFE_RADIO_PACKET_SIZE]);          /* :158-171 */
int afe_radio_create_position_command(uint8_t flags, const float pos[3], const float vel[3],
                                      const float acc[3], uint8_t raw_out[AFE_RADIO_PACKET_SIZE]); /* :137-156 */
int afe_radio_create_acceleration_command(uint8_t flags, const float acc[3], float yaw_rate,
                                          uint8_t raw_out[AFE_RADIO_PACKET_SIZE]);   /* :173-187 */
int afe_radio_create_simple_command(int type /* 2 kill | 6 idle */, uint8_t flags,
                                    uint8_t raw_out[AFE_RADIO_PACKET_SIZE]);         /* :123-135 */
int afe_radio_decode(const uint8_t raw[AFE_RADIO_PACKET_SIZE], afe_radio_message *out); /* :189-240 */
typedef struct afe_telemetry_packet {  /* TelemetryPacket::TelemetryPacket, TelemetryPacket.hpp:102-120 */
  uint8_t type;            /* 0 = part 1 (accel gyro motorForces position battVoltage), 1 = part 2 */
  uint8_t packet_number;
  float accel[3], gyro[3], motor_forces[4], position[3], batt_voltage;
  float velocity[3], attitude[3], debug_vals[6];
  uint8_t panic_reason, warnings;
} afe_telemetry_packet;
int afe_telemetry_encode(const afe_telemetry_packet *src, uint8_t out[AFE_TELEMETRY_PACKET_SIZE]);
int afe_telemetry_decode(const uint8_t in[AFE_TELEMETRY_PACKET_SIZE], afe_telemetry_packet *out);
/* SetCommandRadioMsg (Quadcopter_T.hpp:62-67) for the on-device logic: decode
 * `count` consecutive 23-byte packets and apply them to vehicles first..: rates
 * commands enter EXTERNAL_RATES_CONTROL, idle / kill return to zero motor
 * commands; other types are refused with AFE_ERR_INVALID_ARG (those flight
 * modes live in the host-side logic). */
int afe_set_commands_from_radio(afe_engine *e, int64_t first, int64_t count, const uint8_t *raw_packets);

/* ---- batched RAPPIDS depth-image planner --------------
 * The caller on the other side of the step: per vehicle, search random minimum-
 * jerk motion primitives for the lowest-cost one that is input-feasible,
 * velocity-admissible and collision-free against a depth image, exactly as
 * RectangularPyramidPlanner::DepthImagePlanner::FindLowestCostTrajectory
 * (Components/Components/DepthImagePlanner/DepthImagePlanner.cpp:91-212) with
 * RandomTrajectoryGenerator (DepthImagePlanner.hpp:335-432), IsCollisionFree
 * (:214-301), InflatePyramid (:456-970) and RapidTrajectoryGenerator
 * (Components/Components/TrajectoryGenerator/RapidTrajectoryGenerator.cpp:
 * 75-208), with ONE deliberate change: the reference stops after a wall-clock
 * budget (main.cpp:498: 50 ms), which makes the number of candidates
 * nondeterministic; here it is an explicit count.  Everything is double, in the
 * camera-fixed frame (initial position 0; x right, y down, z into the image). */
typedef struct afe_planner_config {
  int width, height;                 /* depth image size [pixels] */
  double depth_scale;                /* metres per count (main.cpp:121-122: 10/256) */
  double focal_length, cx, cy;       /* pinhole intrinsics [pixels] (main.cpp:360,484-488) */
  double true_vehicle_radius;        /* physicalVehicleRadius [m] */
  double planning_vehicle_radius;    /* vehicleRadiusForPlanning [m] */
  double min_checking_dist;          /* minimumCollisionDistance [m] */
  double min_thrust, max_thrust;     /* [m/s^2]; reference defaults 5, 30 (DepthImagePlanner.cpp:43-44) */
  double max_ang_vel;                /* [rad/s]; default 20 */
  double max_velocity;               /* [m/s]; default 5 */
  double min_section_time;           /* [s]; default 0.02; > 0 and above the longest sample's duration / 2^23 (below) */
  int max_pyramids;                  /* per plan (SetMaxNumberOfPyramids); also sizes the scratch */
  int pixel_buffer;                  /* _pyramidSearchPixelBuffer = 2 */
  int cost_type;                     /* 0: ExplorationCost, -dir.pos(T)/T (DepthImagePlanner.hpp:476-506)
                                        1: Rappids_Simulator's goal cost, -(|G|-|G-pos(T)|)/T (main.cpp:86-107) */
  double cost_vec[3];                /* direction or goal (camera frame) when no per-vehicle array is given */
} afe_planner_config;
int afe_planner_default_config(afe_planner_config *out, int width, int height, double depth_scale,
                               double focal_length, double true_vehicle_radius,
                               double planning_vehicle_radius, double min_checking_dist);
typedef struct afe_plan_output {
  int found;            /* FindLowestCostTrajectory's return value */
  int best_index;       /* winning candidate, -1 if none */
  double best_cost;
  double coeffs[6][3];  /* CommonMath::Trajectory of the winner: t^5 .. t^0 (Trajectory.hpp:31-36) */
  double tf;            /* its duration [s] */
  int n_generated, n_cost_checks, n_collision_checks, n_velocity_checks, n_collision_free, n_pyramids;
} afe_plan_output;
/* Candidate end states exactly as RandomTrajectoryGenerator's default constructor
 * draws them from std::mt19937(seed) (DepthImagePlanner.hpp:349-366,393-404, with
 * GCC's right-to-left evaluation of the three arguments): samples[k] = {pixelX,
 * pixelY, depth [m], duration [s]}.  The reference re-seeds with 0 at every call.
 * Pure host. */
int afe_planner_samples(uint32_t seed, int width, int height, int n_candidates, double *samples4);
/* Plan for n vehicles on GPU `device` (< 0: current).  Host arrays:
 *   depth_images [n_images][height][width] uint16; image_index[n] or NULL (image i)
 *   vel0, acc0, grav: planar [3][n]; cost_vec planar [3][n] or NULL (cfg->cost_vec)
 *   samples [n_tables][n_candidates][4]; sample_table[n] or NULL (table 0)
 *   out[n]; flags [n][n_candidates] or NULL: TrajectoryTestResult bits per candidate
 *   (1 LowCost, 2 DynamicsFeasible, 4 VelocityAdmissible, 8 CollisionFree).
 * Image size: ceil(width/64) * height <= 8192 (one bit per pixel is kept in LDS;
 * e.g. 640x480, 1024x512), width * height < 2^24, and width * height *
 * max(width, height) <= 2^32 (the scans' index division is exact up to there;
 * e.g. 8192x64, 2048x256 pass, 9000x56 does not), else AFE_ERR_OUT_OF_RANGE --
 * decided on the host before anything is allocated or launched.
 * cfg->min_section_time: the input-feasibility test halves a candidate's duration
 * until a section is shorter than this, and the kernel holds at most 24 pending
 * halves where the reference recurses without a limit.  So that no candidate can
 * reach that limit, min_section_time <= 0 and max(sample duration) /
 * min_section_time >= 2^23 are refused with AFE_ERR_OUT_OF_RANGE (for 3 s
 * candidates: anything below 0.36 us). */
int afe_rappids_plan(int device, const afe_planner_config *cfg, int64_t n, const uint16_t *depth_images,
                     int64_t n_images, const int32_t *image_index, const double *vel0, const double *acc0,
                     const double *grav, const double *cost_vec, const double *samples, int n_tables,
                     const int32_t *sample_table, int n_candidates, afe_plan_output *out, uint8_t *flags,
                     float *kernel_ms);

/* ---- depth camera --------------------------------------
 * The reference gets its depth image from AirSim/Unity over RPC
 * (Simulator/Rappids_Simulator/main.cpp:332-354: ImageType::DepthVis, 8-bit,
 * widened to uint16; far = 10 m, depthScale = far/256, focal = width/2,
 * :120-122,360) with the camera mounted at depthCamAtt = FromEulerYPR(-90 deg,
 * 0, -90 deg) on the body (:123-125; camera-to-world = att * depthCamAtt,
 * :520).  Neither the renderer nor the orchard scene is in the reference tree,
 * so what is replaced here is that RPC and its image contract: one ray per
 * pixel through ((x - cx)/f, (y - cy)/f, 1) in the camera frame (x right,
 * y down, z forward), closest hit over a triangle mesh, count =
 * min(max_count, floor(z / depth_scale)), max_count for a miss.
 *
 * A scene is a static triangle mesh (world frame, metres) with a bounding-
 * volume hierarchy built on the host and kept in HBM. */
typedef struct afe_scene afe_scene;

typedef struct afe_camera {
  int32_t width, height;
  double focal_length, cx, cy;
  double depth_scale;   /* metres per count */
  int32_t max_count;    /* 255: 8-bit DepthVis */
  int32_t reserved;
} afe_camera;

/* main.cpp's camera: focal = width/2, principal point = centre, 10 m / 256. */
int afe_camera_default(afe_camera *cam, int width, int height);
/* depthCamAtt of main.cpp:123-125 as a quaternion (w, x, y, z). */
int afe_camera_default_mount(double mount[4]);

/* triangles: n_tri x 9 floats (v0, v1, v2).  device < 0: current device. */
int afe_scene_create(int device, const float *triangles, int64_t n_tri, afe_scene **out);
void afe_scene_destroy(afe_scene *s);
/* Pure host (no GPU): builds the hierarchy afe_scene_create would build and verifies it --
 * every triangle in exactly one leaf, every box containing what hangs below it, depth within
 * the traversal stack; returns its node count, depth and largest leaf. */
int afe_scene_check_hierarchy(const float *triangles, int64_t n_tri, int64_t *n_nodes, int *depth, int *max_leaf);
/* n_tri, number of BVH nodes, tree depth, world bounds {min xyz, max xyz} */
int afe_scene_info(const afe_scene *s, int64_t *n_tri, int64_t *n_nodes, int *depth, double bounds[6]);

/* n_views depth images from explicit poses.  pos: planar [3][n_views]
 * doubles, att: planar [4][n_views] (w,x,y,z) body attitudes, mount: body-to-
 * camera mount quaternion applied to every view (NULL = identity, att is then
 * the camera attitude itself).  depth_out: host buffer of n_views * height *
 * width uint16.  kernel_ms (optional): HIP-event time of the render launch. */
int afe_render_depth(afe_scene *s, const afe_camera *cam, int64_t n_views, const double *pos, const double *att,
                     const double mount[4], uint16_t *depth_out, float *kernel_ms);

/* Which form of the traversal the renders of this scene use: 0 (default) -- tiles whose 64 rays agree on
 * the direction signs walk the octant-mirrored copy of the tree (ordered box tests), the others the plain
 * copy; 1 -- every tile takes the plain, sign-agnostic walk.  The images are the same bits either way
 * (tests/test_gpu_render.py renders thousands of views both ways): a cross-check, not a tuning knob. */
int afe_scene_set_walk(afe_scene *s, int mode);

/* What the traversal did for such a batch (a counting build of the same kernel; the images are
 * discarded): stats[0] BVH nodes visited and [1] triangle box tests / [2] double-precision
 * ray-triangle tests executed, per wave of 64 rays; [3], [4] the same two per participating ray;
 * [5] rays; [6] waves; [7] the triangles the tiles really show (distinct closest-hit triangles per wave, summed):
 * the double-precision tests no traversal could avoid.  bench.py states the camera's floor with these. */
int afe_render_depth_stats(afe_scene *s, const afe_camera *cam, int64_t n_views, const double *pos, const double *att,
                           const double mount[4], uint64_t stats[8], float *kernel_ms);

/* The same, with the poses read on the device from the engine's state slabs
 * (vehicles [first, first+count)), replacing client.simGetImages() for every
 * vehicle at once.  depth_out is a DEVICE pointer when out_is_device != 0
 * (count * height * width uint16, e.g. the buffer handed to
 * afe_rappids_plan_device), else a host buffer.  Engine and scene must live on
 * the same device; the launch is ordered on the engine's stream. */
int afe_render_depth_engine(afe_engine *e, afe_scene *s, const afe_camera *cam, int64_t first, int64_t count,
                            const double mount[4], void *depth_out, int out_is_device, float *kernel_ms);

/* ---- mesh clearance and contact monitor -----------------------------------
 * What the reference left to Unity's collision report: how close is every
 * vehicle to the world's triangle mesh, and has it touched it?  A clearance
 * map is a static mesh (world frame, metres) with a hierarchy of its own in
 * HBM -- a second handle beside afe_scene for the same triangles: the camera's
 * tree is laid out for coherent rays, this one for one incoherent point per
 * lane.  Distances are returned SQUARED (the definition uses + - * / only, so
 * that every bit of the answer is specified: csrc/afe_clearance.hip states the
 * expression tree).  The vehicle is a point: compare with the square of its
 * radius.  Contact is reported, the physics does not react to it.
 * A point query sees a vehicle only where it is asked: a monitor updated at
 * 100 Hz sees a vehicle at the planner's 5 m/s limit every 5 cm, against a
 * vehicle radius of 11.6 cm.  What lies between two queries is covered by the
 * swept entries below (afe_clearance_segments,
 * afe_contact_monitor_create_swept, afe_clearance_paths_swept). */
typedef struct afe_clearance_map afe_clearance_map;
/* triangles: n_tri x 9 floats (v0, v1, v2), finite.  device < 0: current device. */
int afe_clearance_map_create(int device, const float *triangles, int64_t n_tri, afe_clearance_map **out);
/* NULL is AFE_ERR_INVALID_ARG.  Destroy the monitors that borrow the map first. */
int afe_clearance_map_destroy(afe_clearance_map *m);
/* n_tri, inner nodes of the hierarchy, its depth, world bounds {min xyz, max xyz} */
int afe_clearance_map_info(const afe_clearance_map *m, int64_t *n_tri, int64_t *n_nodes, int *depth, double bounds[6]);
/* Pure host (no GPU): builds the hierarchy afe_clearance_map_create would build and verifies it -- every triangle
 * in exactly one leaf (or once in the short list of scene-spanning triangles kept out of the tree), every box
 * containing what hangs below it, depth within the traversal stack (32); leaves hold at most 4 triangles. */
int afe_clearance_check_hierarchy(const float *triangles, int64_t n_tri, int64_t *n_nodes, int *depth, int *max_leaf);

/* Explicit points: pos planar [3][n_points] doubles.  Per point: squared distance to the closest point of the mesh,
 * index of that triangle IN THE ORDER GIVEN TO afe_clearance_map_create (lowest index among bitwise-equal distances),
 * and (closest_out != NULL) the closest point, planar [3][n_points].  Only triangles with dist2 <= max_dist*max_dist
 * count (product formed once, in double); a point with none gets dist2 = +inf, index -1, closest = NaN.
 * max_dist = +inf is allowed (plain nearest-triangle query); NaN or <= 0 is AFE_ERR_INVALID_ARG.  A point with a
 * non-finite coordinate is answered +inf / -1 without a walk.  kernel_ms (optional): HIP-event time of the launch. */
int afe_clearance_query(afe_clearance_map *m, int64_t n_points, const double *pos, double max_dist,
                        double *dist2_out, int32_t *tri_out, double *closest_out, float *kernel_ms);
/* What the traversal did for such a batch (a counting build of the same kernel; the answers are discarded), summed
 * over the points: stats[0] tree nodes visited, [1] triangle box tests, [2] double-precision closest-point
 * evaluations, [3] points. */
int afe_clearance_query_stats(afe_clearance_map *m, int64_t n_points, const double *pos, double max_dist,
                              uint64_t stats[4], float *kernel_ms);
/* The same query for vehicles [first, first+count) read on the device from the engine's slabs (fp32 or fp64 state;
 * absolute x = pos_anchor_xy + (double)pos, as the depth camera forms it), ordered on the engine's stream; a
 * resident step grid ends first.  Outputs (dist2: count doubles, tri: count int32, closest: planar [3][count]
 * doubles or NULL) are DEVICE pointers when out_is_device != 0, else host buffers.  Engine and map must live on
 * the same device.  count == 0 with a valid range returns AFE_OK without touching the engine. */
int afe_clearance_query_engine(afe_engine *e, afe_clearance_map *m, int64_t first, int64_t count, double max_dist,
                               void *dist2_out, void *tri_out, void *closest_out, int out_is_device, float *kernel_ms);

/* Path clearance: does a planned trajectory stay clear of the mesh?  A path is a quintic per axis, coeffs[6][3] =
 * t^5 .. t^0 (the layout of afe_plan_output::coeffs), over a time range (t_begin, t_end), optionally placed by an
 * origin o[3] and a row-major matrix R[9]: world point = o + R * p(t).  It is SAMPLED at n_samples = K times, 2 <= K <=
 * 4096 (else AFE_ERR_OUT_OF_RANGE): t_k = t_begin + (t_end - t_begin) * (k / (K - 1)), t_{K-1} = t_end exactly; every
 * sample is answered by the unbounded point query above and the K answers are reduced on the device to one record.
 * csrc/afe_clearance.hip states every operation; tests/path_checker.py restates it.
 *   n_nonfinite   samples with a non-finite coordinate (a NaN is data, not an error; such a sample is never a hit)
 *   n_hit         samples with dist2 <= radius*radius;  k_first_hit the lowest such k (-1: none), tri_first_hit its
 *                 triangle, t_first_hit its time (NaN: none)
 *   min_dist2     the smallest dist2 among the samples with dist2 <= max_dist*max_dist;  k_min the lowest k among
 *                 bitwise-equal minima;  tri_min, closest[3], t_min from that sample.  None: +inf, -1, -1, NaN, NaN.
 * 0 < radius <= max_dist, radius finite, max_dist may be +inf (else AFE_ERR_INVALID_ARG).  max_dist only limits what is
 * reported as the closest approach (and lets the search prune); the hit fields do not depend on it.
 * Between two samples a path can come closer than at both: afe_clearance_paths_swept below measures the chords between
 * the samples instead, and afe_path_chord_deviation bounds how far the curve leaves them. */
typedef struct afe_path_clearance {      /* 8-byte members only, 96 bytes; the layout is ABI */
  double  min_dist2, closest[3], t_min, t_first_hit;
  int64_t k_min, tri_min, k_first_hit, tri_first_hit, n_hit, n_nonfinite;
} afe_path_clearance;

/* Pure host (no GPU): the sample times t_out[K] and world points xyz_out (planar [3][K]) of ONE path by the definition's
 * expressions.  origin3 and rot9 may be NULL (rot9 without origin3: AFE_ERR_INVALID_ARG). */
int afe_path_sample_points(const double *coeffs18, double t_begin, double t_end, const double *origin3,
                           const double *rot9, int n_samples, double *t_out, double *xyz_out);

/* n_paths explicit paths: coeffs [n][6][3]; t_range planar [2][n]; origin planar [3][n] or NULL; rot planar [9][n] or
 * NULL (rot without origin: AFE_ERR_INVALID_ARG).  out: n_paths records.  n_colliding (optional): the number of paths
 * with n_hit > 0, summed on the device.  n_paths == 0 is AFE_OK.  kernel_ms (optional): HIP-event time of the launch. */
int afe_clearance_paths(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range,
                        const double *origin, const double *rot, int n_samples, double radius, double max_dist,
                        afe_path_clearance *out, int64_t *n_colliding, float *kernel_ms);
/* What the traversal did for such a batch (a counting build of the same kernel; the records are discarded), summed over
 * the samples: stats[0] tree nodes visited, [1] triangle box tests, [2] double-precision closest-point evaluations,
 * [3] samples (n_paths * n_samples). */
int afe_clearance_paths_stats(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range,
                              const double *origin, const double *rot, int n_samples, double radius, double max_dist,
                              uint64_t stats[4], float *kernel_ms);

/* The plans of vehicles [first, first+count) as afe_rappids_plan* returned them (camera frame): origin = the vehicle's
 * position, rot = the camera-to-world matrix of att * mount (NULL mount: identity), both read on the device from the
 * engine's slabs with the depth camera's arithmetic; the time range is [0, tf].  A plan with found == 0 is not sampled:
 * its record is the empty one (+inf, every index -1, NaNs, both counts 0).  The plans are the only upload; the call is
 * ordered on the engine's stream, a resident step grid ends first, engine and map must live on the same device.
 * count == 0 with a valid range returns AFE_OK without touching the engine.  Calls on one map take turns. */
int afe_clearance_plans_engine(afe_engine *e, afe_clearance_map *m, int64_t first, int64_t count,
                               const double mount[4], const afe_plan_output *plans, int n_samples,
                               double radius, double max_dist, afe_path_clearance *out,
                               int64_t *n_colliding, float *kernel_ms);

/* ---- swept clearance: the exact squared distance between a SEGMENT P0 -> P1 and the mesh, with the point query's
 * contract (IEEE double, + - * / and comparisons in a stated order, no output bit depends on the hierarchy):
 * csrc/afe_clearance.hip states the definition (SWEPT CLEARANCE), tests/swept_checker.py restates it.  Per triangle the
 * candidates are 0: P0, 1: P1, 2: the point where the segment crosses the triangle's plane, 3/4/5: the segment against
 * the sides AB/AC/BC; the smallest wins, the earliest among equals.  A segment of zero length is the point query, bit for
 * bit.  A pierced triangle gives a dist2 like 1e-30, not necessarily 0.  Meant for tick-to-tick motion and the chords of a
 * sampled path: the search bounds a segment by its axis-aligned box, which is loose for a long diagonal segment -- that
 * costs time, never bits. */
typedef struct afe_segment_clearance {   /* 48 bytes; the layout is ABI */
  double  dist2;        /* +inf: no triangle within max_dist, or a non-finite coordinate */
  double  s;            /* parameter of the closest point on the segment, P0 + (P1 - P0) * s  (NaN: none) */
  double  closest[3];   /* the closest point on the triangle (NaN: none) */
  int32_t tri;          /* index in the order given to afe_clearance_map_create (-1: none) */
  int32_t kind;         /* the winning candidate, 0 .. 5 (-1: none) */
} afe_segment_clearance;
/* n explicit segments: p0, p1 planar [3][n] doubles; out: n records.  max_dist as afe_clearance_query.  n == 0 is AFE_OK. */
int afe_clearance_segments(afe_clearance_map *m, int64_t n, const double *p0, const double *p1, double max_dist,
                           afe_segment_clearance *out, float *kernel_ms);
/* The counting build for such a batch (the records are discarded): stats[0] tree nodes visited, [1] triangle box tests,
 * [2] double-precision segment evaluations, [3] segments. */
int afe_clearance_segments_stats(afe_clearance_map *m, int64_t n, const double *p0, const double *p1, double max_dist,
                                 uint64_t stats[4], float *kernel_ms);

/* afe_path_clearance over CHORDS: the sample points w_k are those of afe_clearance_paths, chord k is (w_k, w_k+1) for
 * k = 0 .. K-2, every chord is answered by the unbounded segment query.  The fields mean what they mean there, with
 * "chord" for "sample"; a chord with a non-finite end is counted in n_nonfinite and is never a hit.  s_min and
 * s_first_hit are the segment parameters of the closest points, t_min and t_first_hit their times
 * t_k + (t_k+1 - t_k) * s. */
typedef struct afe_path_sweep {          /* 8-byte members only, 112 bytes; the layout is ABI */
  double  min_dist2, closest[3], t_min, t_first_hit;
  int64_t k_min, tri_min, k_first_hit, tri_first_hit, n_hit, n_nonfinite;
  double  s_min, s_first_hit;
} afe_path_sweep;
/* The swept siblings of afe_clearance_paths, afe_clearance_paths_stats (stats[3]: chords, n_paths * (n_samples - 1)) and
 * afe_clearance_plans_engine: the same arguments, the same refusals, afe_path_sweep records. */
int afe_clearance_paths_swept(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range,
                              const double *origin, const double *rot, int n_samples, double radius, double max_dist,
                              afe_path_sweep *out, int64_t *n_colliding, float *kernel_ms);
int afe_clearance_paths_swept_stats(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range,
                                    const double *origin, const double *rot, int n_samples, double radius,
                                    double max_dist, uint64_t stats[4], float *kernel_ms);
int afe_clearance_plans_engine_swept(afe_engine *e, afe_clearance_map *m, int64_t first, int64_t count,
                                     const double mount[4], const afe_plan_output *plans, int n_samples,
                                     double radius, double max_dist, afe_path_sweep *out,
                                     int64_t *n_colliding, float *kernel_ms);
/* Pure host (no GPU): an upper bound, in metres, on how far the quintic leaves the polyline of its n_samples sample
 * points: h*h/8 * max|p''| with h = |t_end - t_begin| / (K - 1) and |p''| bounded per axis by
 * sum_j |c_j| (5-j)(4-j) T^(3-j), T = max(|t_begin|, |t_end|), the axes combined by the Euclidean norm, times the
 * Frobenius norm of rot9 if given, rounded up by 1 + 2^-40.  sqrt(min_dist2) of the swept audit minus this bound is a
 * clearance the CURVE keeps.  The bound is crude (triangle inequalities throughout) and not tuned. */
int afe_path_chord_deviation(const double *coeffs18, double t_begin, double t_end, const double *rot9, int n_samples,
                             double *bound_m);

/* ---- image truth: the planner's own self-evaluation (DepthImagePlanner.cpp:1031-1098 IsCollisionFreeGroundTruth and
 * :972-1002 MeasureConservativeness, Section IV.A of the RAPPIDS paper) --------------------------------------------
 * Against the depth image the planner saw: a path (coeffs[6][3] = t^5 .. t^0, the layout of afe_plan_output::coeffs,
 * camera frame, over [t_begin, t_end)) is sampled at t_0 = t_begin, t_{k+1} = t_k + timestep while t_k < t_end (the
 * reference's running sum; it uses timestep = 0.1).  Samples nearer than cfg->min_checking_dist are skipped.  First
 * every sample's projection must keep edge = int(f * true_vehicle_radius / min_checking_dist) pixels from the image
 * border (else verdict 1: out of view, at the lowest such sample, and no pixel is looked at); then, sample by sample,
 * every pixel deeper than ignore = uint16(true_vehicle_radius / depth_scale) whose ray meets the sphere of
 * planning_vehicle_radius about the sample must lie behind it (else verdict 2: occluded, at the first such sample;
 * pixel_hit = the lowest y*width + x among its occluding pixels).  Verdict 0: free.  csrc/afe_truth.hip states every
 * operation, tests/truth_checker.py restates it; the two agree bit for bit.
 *   n_samples   K (more than 4096: AFE_ERR_OUT_OF_RANGE)
 *   n_checked   samples whose pixels were examined, up to and including k_hit (0 with verdict 1)
 *   absent fields are -1 / NaN;  the empty record (a plan with found == 0): verdict -1, every index -1, NaNs, counts 0
 * Refused before any launch, outputs untouched: NULLs, width or height <= 0, timestep not finite or <= 0, a device
 * image pointer that is not 16-byte aligned, fewer images than paths without image_index (AFE_ERR_INVALID_ARG);
 * width*height > 2^24, min_checking_dist <= 0, true_vehicle_radius / depth_scale not in (-1, 65536), an edge beyond
 * 2^30, an image_index entry outside [0, n_images), K > 4096 (AFE_ERR_OUT_OF_RANGE).
 * What sampling does NOT cover: between two samples a path can be occluded where it is free at both. */
typedef struct afe_image_truth {         /* 8-byte members only, 64 bytes; the layout is ABI */
  int64_t verdict, k_fov;
  double  t_fov;
  int64_t k_hit;
  double  t_hit;
  int64_t pixel_hit, n_samples, n_checked;
} afe_image_truth;
typedef struct afe_conservativeness {    /* MeasureConservativeness' tally; 8-byte members only, 48 bytes */
  int64_t n_checked;                /* candidates the planner collision-checked (flag bit 4 set) */
  int64_t n_planner_free;           /* of those: the planner calls them collision-free (flag bit 8 set) */
  int64_t n_correct_in_collision;   /* the planner rejects, the ground truth too (verdict != 0) */
  int64_t n_incorrect_in_collision; /* the planner rejects, the ground truth calls it free (verdict == 0) */
  int64_t n_free_but_out_of_view;   /* the planner accepts, verdict 1 */
  int64_t n_free_but_occluded;      /* the planner accepts, verdict 2 */
} afe_conservativeness;

/* Pure host (no GPU): the definition's sample count and, if t_out is not NULL, the times t_out[*n_samples] (room for
 * 4096).  K > 4096: AFE_ERR_OUT_OF_RANGE, nothing written. */
int afe_image_truth_sample_times(double t_begin, double t_end, double timestep, int *n_samples, double *t_out);

/* n_paths explicit paths on GPU `device` (< 0: current): coeffs [n][6][3]; t_range planar [2][n].  images
 * [n_images][height][width] uint16: a host array, or (images_on_device != 0) a 16-byte-aligned device pointer, e.g.
 * what afe_render_depth_engine filled.  image_index [n_paths] (host) or NULL (image i for path i).  out: n_paths
 * records.  n_free (optional): the number of records with verdict 0, summed on the device.  n_paths == 0 is AFE_OK. */
int afe_image_truth_paths(int device, const afe_planner_config *cfg, int64_t n_paths, const void *images,
                          int64_t n_images, int images_on_device, const int32_t *image_index, const double *coeffs,
                          const double *t_range, double timestep, afe_image_truth *out, int64_t *n_free,
                          float *kernel_ms);
/* What the scan did for such a batch (a counting build of the same kernel; the records are discarded): stats[0]
 * samples whose pixels were examined, [1] pixels tested for s, [2] pixels whose ray met the sphere (s >= 0),
 * [3] width * height * stats[0], what visiting every pixel would have tested. */
int afe_image_truth_paths_stats(int device, const afe_planner_config *cfg, int64_t n_paths, const void *images,
                                int64_t n_images, int images_on_device, const int32_t *image_index,
                                const double *coeffs, const double *t_range, double timestep, uint64_t stats[4],
                                float *kernel_ms);
/* The plans afe_rappids_plan* returned, each over [0, tf); found == 0 gives the empty record. */
int afe_image_truth_plans(int device, const afe_planner_config *cfg, int64_t n, const void *images, int64_t n_images,
                          int images_on_device, const int32_t *image_index, const afe_plan_output *plans,
                          double timestep, afe_image_truth *out, int64_t *n_free, float *kernel_ms);
/* MeasureConservativeness for n planners x n_candidates candidates: vel0, acc0, samples, sample_table as given to
 * afe_rappids_plan*, flags [n][n_candidates] as it filled them.  EVERY candidate is formed (by the planner's own
 * functions: coeffs_out [n][n_candidates][6][3], optional, holds what was judged) and judged over [0, duration):
 * verdict_out [n][n_candidates] bytes.  Only candidates the planner collision-checked (flag bit 4) are tallied, on the
 * device, in integers: tally = the sum over all planners, per_planner [n] (optional) each planner's own. */
int afe_image_truth_candidates(int device, const afe_planner_config *cfg, int64_t n, const void *images,
                               int64_t n_images, int images_on_device, const int32_t *image_index,
                               const double *vel0, const double *acc0, const double *samples, int n_tables,
                               const int32_t *sample_table, int n_candidates, const uint8_t *flags, double timestep,
                               uint8_t *verdict_out, double *coeffs_out, afe_conservativeness *tally,
                               afe_conservativeness *per_planner, float *kernel_ms);

/* Per-vehicle latches, device resident, for a closed loop that wants to know about contact without downloading
 * the state: 0 < contact_radius <= search_radius, both finite.  The monitor BORROWS engine and map: destroy it
 * before either of them (not tracked). */
typedef struct afe_contact_monitor afe_contact_monitor;
int afe_contact_monitor_create(afe_engine *e, afe_clearance_map *m, double contact_radius, double search_radius,
                               afe_contact_monitor **out);
/* One query (max_dist = search_radius) at the engine's current state and time (afe_time_us); updates, per vehicle:
 * the smallest dist2 seen so far over the updates (+inf while nothing came within search_radius), and -- the first
 * time dist2 <= contact_radius^2 -- the time and the triangle index of that update.  Returns how many vehicles
 * are in contact now and how many ever were: two integers summed on the device, the only bytes that cross the
 * bus.  Nothing is allocated here. */
int afe_contact_monitor_update(afe_contact_monitor *c, int64_t *n_in_contact, int64_t *n_ever_in_contact);
/* the latches of vehicles [first, first+count) (any output may be NULL): first_contact_us is UINT64_MAX and
 * first_contact_tri -1 for a vehicle that never made contact */
int afe_contact_monitor_get(afe_contact_monitor *c, int64_t first, int64_t count, double *min_dist2,
                            uint64_t *first_contact_us, int32_t *first_contact_tri);
/* back to "nothing seen" for vehicles [first, first+count) */
int afe_contact_monitor_reset(afe_contact_monitor *c, int64_t first, int64_t count);
int afe_contact_monitor_destroy(afe_contact_monitor *c);   /* NULL is AFE_ERR_INVALID_ARG */
/* The SWEPT monitor: the same handle type, served by the same _update/_get/_reset/_destroy.  It keeps every vehicle's
 * previous world position on the device (the double the last update itself formed) and an update measures the segment
 * from there to the current position, so an obstacle thinner than the distance flown between two updates is not missed.
 * A vehicle's first update after creation or _reset (and after an update that found its position non-finite) measures
 * the zero-length segment: exactly the point monitor's answer.  first_contact_us is the time of the update whose
 * segment came within the radius.  _reset also forgets the previous position: reset the vehicles you move with
 * afe_set_state, or the jump is measured as a flight. */
int afe_contact_monitor_create_swept(afe_engine *e, afe_clearance_map *m, double contact_radius, double search_radius,
                                     afe_contact_monitor **out);

/* ---- range beams: what one arbitrary ray hits first, and how far away -------------------------------------------
 * On the clearance map's own tree.  csrc/afe_raycast.hip states the definition, tests/raycast_checker.py restates it
 * in numpy; the two agree bit for bit and no output bit depends on the hierarchy.  IEEE double, contraction off.
 *   One ray (origin o, direction d, neither normalised) against one triangle: the depth camera's closed, watertight
 *   rule (the one behind afe_render_depth and its CPU checker, operation for operation): v0, e1 = v1 - v0, e2 = v2 - v0 in
 *   double; p = d x e2; det = e1.p; tv = o - v0; en = max(|e1|_1, |e2|_1); dn = |d|_1;
 *   eps = (dn * (2^-48 * en)) * (|tv|_1 + en); miss unless |det| > eps * max(1, 32768 en); s = sign(det);
 *   nu = (tv.p) s, miss if nu < -eps; q = tv x e1; nv = (d.q) s, miss if nv < -eps; miss if (|det| - nu) - nv < -eps;
 *   t = (e2.q) * (1 / det); a hit iff t > 0.  The map's degenerate flag is not consulted.
 *   WINNER: only hits with t <= t_max count (+inf: no limit); the smallest t wins, among bitwise-equal t the lowest
 *   index in the order given to afe_clearance_map_create.  No hit: (+inf, -1).  A ray with a non-finite component in
 *   o or d: the same, without a walk.  d = 0 hits nothing.  An origin ON a triangle does not hit it (t > 0).
 * t is the ray PARAMETER: metres when |d|_2 = 1.
 * afe_raycast: n rays, origin and dir planar [3][n] doubles, t_max [n] or NULL (no limit); t_out [n], tri_out [n].
 * Refused: NULLs, n < 0 (AFE_ERR_INVALID_ARG); a t_max entry that is NaN or negative, n > 2^40 (AFE_ERR_OUT_OF_RANGE).
 * n == 0 is AFE_OK with no launch. */
int afe_raycast(afe_clearance_map *m, int64_t n, const double *origin, const double *dir, const double *t_max,
                double *t_out, int32_t *tri_out, float *kernel_ms);
/* The counting build for such a batch, a second compilation of the same walk: stats[0] tree nodes visited, [1] triangle
 * box tests, [2] double-precision ray/triangle tests, [3] rays.  t_out and tri_out may be NULL; given, they receive the
 * answers, which are afe_raycast's.  n <= 0 is AFE_ERR_INVALID_ARG. */
int afe_raycast_stats(afe_clearance_map *m, int64_t n, const double *origin, const double *dir, const double *t_max,
                      double *t_out, int32_t *tri_out, uint64_t stats[4], float *kernel_ms);
/* Line of sight from p0 to p1 (planar [3][n] doubles): d = p1 - p0 per axis; blocked[i] = 1 iff the first-hit query
 * with o = p0 and t_max = 1 has a hit, else 0 (a triangle touched at t = 1 exactly blocks; p0 == p1 never does; a
 * non-finite end gives 0).  Served by the first-hit kernel or by one that stops at the first hit with t <= 1: the
 * answer is the same.  n == 0 is AFE_OK. */
int afe_line_of_sight(afe_clearance_map *m, int64_t n, const double *p0, const double *p1, uint8_t *blocked,
                      float *kernel_ms);

/* A RANGE SENSOR on an engine: a mount quaternion (sensor frame in the body frame, like the camera's; NULL: identity)
 * and 1 .. 32 beams.  The vehicle's origin o_v and matrix R are those of the camera pose (att * mount; anchors added in
 * double; fp32 or fp64 slabs; R is not normalised).  Per beam:
 *   frame 0 (sensor frame):  origin w.x = o_v.x + ((R0*off.x + R1*off.y) + R2*off.z), rows 1 and 2 for y and z;
 *                            direction d.x = (R0*dir.x + R1*dir.y) + R2*dir.z, likewise
 *   frame 1 (world frame, a levelled beam such as height above canopy):  w = o_v + off per axis, d = dir
 * then the first-hit query with the beam's t_max (+inf: no limit).  t is in metres when |dir|_2 = 1 and the
 * quaternions are unit.  A vehicle with a non-finite position or attitude reads (+inf, -1) on every beam. */
typedef struct afe_range_beam {          /* 64 bytes; the layout is ABI */
  double  off[3], dir[3], t_max;
  int32_t frame, reserved;
} afe_range_beam;
typedef struct afe_range_sensor afe_range_sensor;
/* Refused: NULLs, non-finite mount, off or dir (AFE_ERR_INVALID_ARG); n_beams outside 1 .. 32, a t_max that is NaN or
 * negative, a frame other than 0 or 1 (AFE_ERR_OUT_OF_RANGE); then the engine's gate; then a map on another device than
 * the engine (AFE_ERR_INVALID_ARG).  The sensor BORROWS engine and map: destroy it before either of them. */
int afe_range_sensor_create(afe_engine *e, afe_clearance_map *m, const double mount[4], const afe_range_beam *beams,
                            int n_beams, afe_range_sensor **out);
/* Vehicles [first, first + count) at the engine's current state: t_out [n_beams][count] doubles, tri_out
 * [n_beams][count] int32 (may be NULL); device pointers if out_is_device, else host arrays.  Ordered on the engine's
 * stream; a resident step grid ends first.  With device outputs and kernel_ms == NULL the call does not wait.
 * count == 0 with a valid range returns AFE_OK without touching the engine; a range beyond the engine is
 * AFE_ERR_OUT_OF_RANGE. */
int afe_range_sensor_update(afe_range_sensor *s, int64_t first, int64_t count, void *t_out, void *tri_out,
                            int out_is_device, float *kernel_ms);
int afe_range_sensor_info(const afe_range_sensor *s, int *n_beams, int64_t *n_vehicles);
int afe_range_sensor_destroy(afe_range_sensor *s);   /* NULL is AFE_ERR_INVALID_ARG */

/* ---- ensemble statistics ---------------------------------------------------
 * What a Monte-Carlo sweep ends with: the distribution of the ensemble's state
 * per parameter bin, now and over the flight, without downloading the state.
 * A statistics monitor reads the engine's slabs on the device (it never writes
 * one), keeps per-vehicle latches resident and returns one record per GROUP of
 * vehicles.  Groups are contiguous index ranges given by n_groups + 1
 * non-decreasing edges, 0 <= edges[0], edges[n_groups] <= n_vehicles; group g is
 * [edges[g], edges[g+1]); 1 <= n_groups <= 65536; empty groups are allowed and
 * vehicles outside every group are never read or written.
 * Every value is specified operation by operation in csrc/afe_stats.hip (IEEE
 * double, + - * and comparisons only; sums in a fixed tree, so no result
 * depends on grid shape or scheduling).  Per vehicle, against its reference
 * point (rx, ry, rz):  dx = X - rx, dy = Y - ry, dz = Z - rz with X, Y, Z as
 * afe_get_state forms them;  h2 = dx*dx + dy*dy;  v2 and w2 the squared speed
 * and body rate;  up = R[8] of the attitude (cosine of the tilt);  valid = the
 * 13 state values and dx, dy, dz are finite;  grounded = valid and Z <= 0.
 * Indices are engine-local.  Not covered: merging records across shards. */
typedef struct afe_stats_monitor afe_stats_monitor;
typedef struct afe_group_stats {          /* 8-byte members only; the layout is ABI */
  int64_t count, n_invalid, n_grounded;            /* now; count = edges[g+1] - edges[g] */
  int64_t n_ever_invalid, n_ever_grounded;         /* latches */
  int64_t sum_n_valid;                             /* over the group, of the per-vehicle update counts */
  int64_t argmax_h2, argmax_peak_h2;               /* lowest index among equal values; -1 with no candidate */
  double sum_h2, sum_dz, sum_dz2, sum_v2, sum_w2;  /* tree sums over the valid vehicles, now */
  double max_h2, min_dz, max_dz, max_v2, max_w2, min_up;   /* over the valid vehicles, now; -inf / +inf with none */
  double sum_peak_h2, sum_acc_h2;                  /* tree sums over every vehicle's latch */
  double max_peak_h2, min_min_up;                  /* over every vehicle's latch */
} afe_group_stats;

/* Pure host (no GPU): validates the edges against n_vehicles; n_chunks = sum over groups of ceil(size / 256),
 * levels = depth of the deepest group's summation tree (ceil(log2(size)); 0 for sizes 0 and 1).  NULL edges, n_groups
 * outside 1..65536, a negative or decreasing edge: AFE_ERR_INVALID_ARG; an edge beyond n_vehicles:
 * AFE_ERR_OUT_OF_RANGE.  The outputs may be NULL. */
int afe_stats_check_layout(const int64_t *edges, int n_groups, int64_t n_vehicles, int64_t *n_chunks, int *levels);

/* Latches initial, reference = where each vehicle is now.  The monitor BORROWS the engine: destroy it first. */
int afe_stats_create(afe_engine *e, const int64_t *edges, int n_groups, afe_stats_monitor **out);
int afe_stats_destroy(afe_stats_monitor *m);   /* NULL is AFE_ERR_INVALID_ARG */
int afe_stats_info(const afe_stats_monitor *m, int *n_groups, int64_t *n_vehicles, int *n_hist_edges, uint64_t *n_updates);
/* Reference points of vehicles [first, first+count): pos3 planar [3][count], finite (else AFE_ERR_INVALID_ARG);
 * NULL: mark where they are now, on the device.  count == 0 with a valid range is AFE_OK without touching the engine. */
int afe_stats_set_reference(afe_stats_monitor *m, int64_t first, int64_t count, const double *pos3);
/* Histogram of the horizontal deviation per group: up to 63 ascending finite edges > 0 in metres (else
 * AFE_ERR_INVALID_ARG); a valid vehicle falls into bin #{k : edges_m[k]^2 <= h2}.  n_edges == 0 (edges_m may be NULL): off. */
int afe_stats_set_histogram(afe_stats_monitor *m, const double *edges_m, int n_edges);
/* One pass over the grouped vehicles at the engine's current state and time (afe_time_us), on the engine's stream (a
 * resident step grid ends first): updates the latches and writes n_groups records to groups_out and, if hist_out is
 * not NULL, int64 counts [n_groups][n_edges + 1] (hist_out without a histogram is AFE_ERR_INVALID_ARG).  Nothing is
 * allocated; the records and the histogram are the only bytes that cross the bus, in one copy. */
int afe_stats_update(afe_stats_monitor *m, afe_group_stats *groups_out, int64_t *hist_out);
/* The latches of vehicles [first, first+count) (any output may be NULL): peak_h2 = largest h2 seen (initially 0),
 * min_up = smallest up seen (+inf), acc_h2 = sum of h2 over the updates (0), n_valid = updates in which the vehicle was
 * valid, first_grounded_us / first_invalid_us = afe_time_us of the first update that found it grounded / not valid
 * (UINT64_MAX: never). */
int afe_stats_get(afe_stats_monitor *m, int64_t first, int64_t count, double *peak_h2, double *min_up, double *acc_h2,
                  int64_t *n_valid, uint64_t *first_grounded_us, uint64_t *first_invalid_us);
/* latches of vehicles [first, first+count) back to initial; the reference stays */
int afe_stats_reset(afe_stats_monitor *m, int64_t first, int64_t count);

/* Device scratch helpers for hosts without their own HIP allocator (ctypes). */
int afe_device_alloc(int device, uint64_t bytes, void **out);
int afe_device_free(void *p);
int afe_device_download(void *host_dst, const void *dev_src, uint64_t bytes);
int afe_device_upload(void *dev_dst, const void *host_src, uint64_t bytes);   /* e.g. depth images for afe_image_truth_* */

/* The planner keeps its device scratch between calls (grown on demand, one set per process; plan calls take
 * turns on it).  This gives the memory back; the next call allocates again. */
int afe_planner_release_scratch(void);

/* afe_rappids_plan with the depth images already in HBM (one per planner, or
 * indexed through image_index, which stays a host array).  The pointer must be
 * 16-byte aligned (anything from afe_device_alloc / hipMalloc is). */
int afe_rappids_plan_device(int device, const afe_planner_config *cfg, int64_t n, const void *dev_depth_images,
                            int64_t n_images, const int32_t *image_index, const double *vel0, const double *acc0,
                            const double *grav, const double *cost_vec, const double *samples, int n_tables,
                            const int32_t *sample_table, int n_candidates, afe_plan_output *out, uint8_t *flags,
                            float *kernel_ms);

/* ---- trajectory follower ----------------------------------------------------
 * The offboard side of the radio for a whole ensemble, on the device: what the
 * Rappids_Simulator loop does between the planner's answer and the vehicle's
 * command radio (Simulator/Rappids_Simulator/main.cpp:490-495,518-528,558-673,
 * 737-739), one lane per vehicle, with the true state standing in for estState
 * unless an estimator is attached (afe_follower_attach_estimator).
 * A follower keeps per vehicle the adopted plan (the 18 coefficients of
 * afe_plan_output::coeffs, its duration, when and in which frame it was
 * planned), a hold position, a goal, previousThrust, the last command before
 * and after the radio codec and the messages in flight.  Nothing of the state is
 * downloaded: a tick reads the engine's slabs and writes the engine's rates
 * command, with exactly the effect of afe_set_rates_commands.
 * Every value is specified operation by operation in csrc/afe_follower.hip
 * (tests/follower_checker.py restates it in numpy): IEEE arithmetic without
 * contraction in the reference's order and precision -- double for the
 * reference, float for the controller, Vec3f(double) narrowings where
 * QuadcopterController.cpp has them -- so that everything but sinf, cosf, asinf,
 * acosf and acos is reproducible to the bit on a host.
 * Not covered: ctrl.Run's take-off branch, the safety net, a desired yaw other
 * than 0 (the flight stage machine below has all three), delivery between ticks.
 * Indices are engine-local.  The follower BORROWS the engine (destroy the
 * follower first) and needs one whose state is in device memory (afe_create). */
typedef struct afe_follower afe_follower;
typedef struct afe_follower_config {
  size_t struct_bytes;          /* IN: sizeof(afe_follower_config) as the caller was compiled; less is AFE_ERR_INVALID_ARG */
  uint64_t period_us;           /* offboard period, main.cpp:175 (100 Hz): 10 000 */
  uint64_t delay_us;            /* command radio delay, main.cpp:178,282-283: 30 000 */
  double lookahead_s;           /* main.cpp:567: 0.04 */
  double omega_step_s;          /* main.cpp:601: 0.02 */
  double mount[4];              /* depthCamAtt, afe_camera_default_mount */
  float nat_freq, damping;      /* posControl_natFreq, posControl_damping (QuadcopterConstants.hpp:34-35) */
  float att_time_const_xy;      /* attControl_timeConst_xy, derived in float as QuadcopterConstants.hpp does */
  float att_time_const_z;       /* attControl_timeConst_z: (0.04f * 5) * 2 = 0.399999976 for type 5, not 0.4f */
  double hover_thrust;          /* reference thrust of a vehicle without a plan [m/s^2]: 9.81 */
} afe_follower_config;

/* QuadcopterController::SetParameters as main.cpp:227-229 calls it for the type (1, 2, 4, 5; else
 * AFE_ERR_INVALID_ARG), and the loop's constants.  Pure host. */
int afe_follower_default_config(int quadcopter_type, afe_follower_config *cfg);
/* Slots of the delay ring: delay_us / period_us + 2 (the messages in flight at a tick, and the one being written).
 * period_us == 0 and a result above 16: AFE_ERR_OUT_OF_RANGE.  Pure host. */
int afe_follower_ring_slots(uint64_t period_us, uint64_t delay_us, int *slots);
/* Nobody has a plan; hold and goal = where each vehicle is now; previousThrust = hover_thrust; nothing in flight.
 * Needs afe_set_rates_logic (else AFE_ERR_NOT_CONFIGURED); a delay that needs more than 16 slots is AFE_ERR_OUT_OF_RANGE. */
int afe_follower_create(afe_engine *e, const afe_follower_config *cfg, afe_follower **out);
int afe_follower_destroy(afe_follower *f);   /* NULL is AFE_ERR_INVALID_ARG */
/* (any output may be NULL) ticks so far, messages in flight after the last tick */
int afe_follower_info(const afe_follower *f, int64_t *n_vehicles, int *slots, uint64_t *n_ticks, int *in_flight);

/* desiredPosition of a vehicle without a plan (main.cpp:561-564) and the point the planner's cost pulls towards
 * (ExplorationCost's direction: goal - position, in the camera frame), world frame, pos3 planar [3][count].
 * count == 0 with a valid range is AFE_OK without touching the engine. */
int afe_follower_set_hold(afe_follower *f, int64_t first, int64_t count, const double *pos3);
int afe_follower_set_goal(afe_follower *f, int64_t first, int64_t count, const double *pos3);
/* The adopted plans of vehicles [first, first+count), for a host-side planner to hand plans in and for read-back: planned
 * uint8 [count], coeffs planar [18][count] (row k = coeffs[k / 3][k % 3]), tf [count], t_plan_us [count] (afe_time_us
 * when it was planned: trackTrajTime.Reset()), traj_att4 planar [4][count] (trajAtt = att * depthCamAtt, main.cpp:520),
 * offset3 (trajOffset, :523) and grav3 (gravity in the plan's frame, :494) planar [3][count].  An array that is NULL is
 * left alone / not read back; all of them NULL is AFE_ERR_INVALID_ARG. */
int afe_follower_set_plans(afe_follower *f, int64_t first, int64_t count, const uint8_t *planned, const double *coeffs,
                           const double *tf, const uint64_t *t_plan_us, const double *traj_att4, const double *offset3,
                           const double *grav3);
int afe_follower_get_plans(afe_follower *f, int64_t first, int64_t count, uint8_t *planned, double *coeffs, double *tf,
                           uint64_t *t_plan_us, double *traj_att4, double *offset3, double *grav3);

/* The planner's inputs of every vehicle as they are now (main.cpp:490-495), formed on the device in double through the
 * rotation matrix of Rotation.hpp:196-220 with camAtt = att * mount: vel0, acc0 (thrust previousThrust along body z,
 * less gravity), grav and the goal vector, planar [3][n] each (any may be NULL, not all). */
int afe_follower_planner_inputs(afe_follower *f, double *vel0, double *acc0, double *grav, double *cost_vec);
/* main.cpp:484-528 for every vehicle: the inputs above, afe_rappids_plan_device on them without their leaving the device
 * (image i for vehicle i, one candidate table samples[n_candidates][4]), and the adoption -- a vehicle whose planner
 * found a trajectory takes its coefficients and duration, t_plan_us = afe_time_us, trajAtt = att * mount, trajOffset =
 * position and the gravity vector, all as they stood for the inputs; the others keep what they had.  out[n] and flags
 * [n][n_candidates] may be NULL (then they are not downloaded); n_found comes back as one 8-byte download. */
int afe_follower_plan(afe_follower *f, const afe_planner_config *cfg, const void *dev_depth_images, const double *samples,
                      int n_candidates, afe_plan_output *out, uint8_t *flags, int64_t *n_found, float *kernel_ms);

/* One offboard period (main.cpp:558-673,737-739), once per period_us after afe_step; the caller keeps the 100 Hz gate.
 * At now = afe_time_us, on the engine's stream (a resident step grid ends first): the tracking reference (:558-608),
 * QuadcopterController::RunTracking (QuadcopterController.cpp:76-132), CreateRatesCommand and its decoding
 * (RadioTypes.hpp:73-116,158-171,218-226) and CommunicationsDelay (CommunicationsDelay.hpp:18-33): the message is queued
 * with due = now + delay_us, every message with due <= now is delivered in send order, and the newest of them is left
 * in the engine's rates command exactly as afe_set_rates_commands would leave it.  Messages are delivered AT TICKS ONLY:
 * one that falls due between two ticks (a delay that is no multiple of the period) waits for the next tick, where the
 * reference looks at every simulation step.  n_tracking (may be NULL: then nothing is downloaded and the call does not
 * wait): vehicles that are on a running plan.  A tick that would leave more messages in flight than the ring holds
 * (ticks closer together than period_us) is AFE_ERR_OUT_OF_RANGE. */
int afe_follower_tick(afe_follower *f, int64_t *n_tracking);

/* What the last tick tracked and commanded.  ref14 planar [14][count]: position 3, velocity 3, acceleration 3, thrust,
 * body rates 3, running (0 / 1).  computed4 / sent4 planar [4][count] (either may be NULL): thrust and body rates before
 * and after the radio codec. */
int afe_follower_get_reference(afe_follower *f, int64_t first, int64_t count, double *ref14);
int afe_follower_get_command(afe_follower *f, int64_t first, int64_t count, float *computed4, float *sent4);
/* Self-test hook: the device library's functions exactly as the follower's kernels call them, on GPU `device` (< 0:
 * current).  op 0..3 = sinf, cosf, asinf, acosf (x, y float [n]); op 4 = acos (x, y double [n]).  With these values a
 * host restatement reproduces every bit of a tick.  Replaces nothing in the reference. */
int afe_follower_selftest_math(int device, int op, int64_t n, const void *x, void *y);

/* ---- mocap state estimator ----------------------------------------------------
 * Offboard::MocapStateEstimator with its PredictionPipe for a whole ensemble, on
 * the device: what stands between the vehicle and the controller in the
 * Rappids_Simulator loop (Simulator/Rappids_Simulator/main.cpp:451-457
 * UpdateWithMeasurement at 200 Hz, :468-469 GetPrediction(0.03), :647-649
 * SetPredictedValues after every controller run).  One constant-velocity filter
 * for the position and one for the attitude per vehicle, propagated between
 * measurements with the commands still in flight.  All double.  Every value is
 * specified by cli/mocap_estimator.hpp line by line (csrc/afe_estimator.hip
 * says how; tests/estimator_checker.py restates it in numpy): IEEE arithmetic
 * without contraction, so that everything but sin, cos, asin, acos and exp is
 * reproducible to the bit on a host.  The reference's own class drops into the
 * same three calls: measure = UpdateWithMeasurement(truth pos, truth att),
 * predict = GetPrediction(ahead), announce = SetPredictedValues.
 * All times are relative to afe_time_us at creation.  The commands in flight are
 * a ring of at most 16 messages for the whole ensemble (every vehicle is
 * announced to in the same call); csrc/afe_estimator_ring.h states its rule.
 * Indices are engine-local.  The estimator BORROWS the engine and needs one whose
 * state is in device memory.  Destroy order: follower, estimator, engine. */
typedef struct afe_estimator afe_estimator;
typedef struct afe_estimator_config {
  size_t struct_bytes;          /* IN: sizeof(afe_estimator_config) as the caller was compiled; less is AFE_ERR_INVALID_ARG */
  double command_delay_s;       /* an announced command is active this much later (main.cpp:178): 0.03 */
  double rate_time_constant_s;  /* the body rates relax towards the command with it (MocapStateEstimator.cpp:24-33): 0.04 */
  double gate;                  /* measurement gate in standard deviations (:181-205): 6 */
  double sigma_pos;             /* measurement noise, position [m]: 0.02 */
  double sigma_att;             /* measurement noise, attitude [rad]: 5 pi / 180 */
  double sigma_acc;             /* process noise, acceleration [m/s^2]: 9.81 */
  double sigma_ang_acc;         /* process noise, angular acceleration [rad/s^2]: 200 */
  uint64_t offboard_period_us;  /* announces are this far apart: 10 000 */
  uint64_t max_measure_gap_us;  /* measure calls are at most this far apart: 10 000 (the loop's are 5 000) */
} afe_estimator_config;

int afe_estimator_default_config(afe_estimator_config *cfg);   /* pure host */
/* Slots of the command ring: (ceil(command_delay_s * 1e6) + 2 * max_measure_gap_us) / offboard_period_us + 3.  A period
 * of 0 or a result above 16: AFE_ERR_OUT_OF_RANGE.  Pure host. */
int afe_estimator_ring_slots(const afe_estimator_config *cfg, int *slots);
/* Reset() for every vehicle at time 0 = afe_time_us now: not started, the zero state, the initial variances, no message. */
int afe_estimator_create(afe_engine *e, const afe_estimator_config *cfg, afe_estimator **out);
int afe_estimator_destroy(afe_estimator *est);   /* NULL is AFE_ERR_INVALID_ARG */
/* (any output may be NULL) measure calls so far, messages in the ring, error: 1 once a propagation loop hit its trip cap
 * of slots + 2 (it cannot with the ring's rule; every later call but this and destroy is then AFE_ERR_OUT_OF_RANGE) */
int afe_estimator_info(const afe_estimator *est, int64_t *n_vehicles, int *slots, uint64_t *n_measures, int *n_messages,
                       uint32_t *error);

/* UpdateWithMeasurement(position, attitude as the engine holds them now) for every vehicle, on the engine's stream (a
 * resident step grid ends first): the first measurement initialises; later ones propagate to now with the commands in
 * flight, gate at `gate` sigma (a rejected measurement is counted and skipped; after ten in a row the filter is reset
 * and takes the eleventh), update and symmetrise.  n_rejected (may be NULL: then nothing is downloaded and the call does
 * not wait): measurements this call rejected. */
int afe_estimator_measure(afe_estimator *est, int64_t *n_rejected);
/* GetPrediction(ahead_s) for every vehicle into the estimator's prediction buffer, stamped with afe_time_us; the
 * estimate itself does not change.  Does not wait. */
int afe_estimator_predict(afe_estimator *est, double ahead_s);
/* The last prediction, est13 planar [13][count]: position 3, velocity 3, attitude 4, body rates 3.  Without a
 * prediction: AFE_ERR_NOT_CONFIGURED. */
int afe_estimator_get_prediction(afe_estimator *est, int64_t first, int64_t count, double *est13);
/* SetPredictedValues from host arrays (a host-side controller), planar [3][count] each: one new message for the WHOLE
 * ensemble, active command_delay_s from now; vehicles outside [first, first+count) repeat the message before it (+0
 * if there is none).  AFE_ERR_OUT_OF_RANGE, and nothing changes, if the activation time is not strictly later than the
 * newest message's, or if the slot to be overwritten may still be needed (csrc/afe_estimator_ring.h). */
int afe_estimator_announce(afe_estimator *est, int64_t first, int64_t count, const double *ang_vel3, const double *acc3);
/* The filter as it stands: est13 as above, cov6 planar [6][count] (position filter vv, vr, rr, attitude filter vv, vr,
 * rr; rv is vr), valid_at_us (the time the estimate is valid at), started, the rejections in a row and in all.  An
 * array that is NULL is not read back; all of them NULL is AFE_ERR_INVALID_ARG. */
int afe_estimator_get_state(afe_estimator *est, int64_t first, int64_t count, double *est13, double *cov6, uint64_t *valid_at_us,
                            uint8_t *started, uint32_t *rejected_in_a_row, uint32_t *rejected);
/* Reset() for vehicles [first, first+count) at the time of the call (the rejection counters stay).  Does not wait. */
int afe_estimator_reset(afe_estimator *est, int64_t first, int64_t count);
/* Self-test hook: the device library's double functions exactly as the estimator's kernels call them, on GPU `device`
 * (< 0: current).  op 0..4 = sin, cos, asin, acos, exp; x, y double [n]. */
int afe_estimator_selftest_math(int device, int op, int64_t n, const double *x, double *y);
/* estState for the follower (main.cpp:468-469): while an estimator is attached (it must borrow the same engine, else
 * AFE_ERR_INVALID_ARG; NULL detaches), afe_follower_planner_inputs, afe_follower_plan (inputs and adoption) and
 * afe_follower_tick read position, velocity and attitude from the estimator's prediction buffer instead of the
 * engine's slabs, and afe_follower_tick announces (cmdAngVel, R(estAtt) e3 cmdThrust - (0, 0, 9.81)) -- the doubles
 * before any narrowing, main.cpp:647-649 -- into the estimator's ring, under announce's refusals.  A tick, plan or
 * planner_inputs without a prediction stamped at the current afe_time_us is AFE_ERR_NOT_CONFIGURED. */
int afe_follower_attach_estimator(afe_follower *f, afe_estimator *est);

/* ---- GPS + IMU state estimator -------------------------------------------------
 * Offboard::GPSIMUStateEstimator (Components/Components/Offboard/GPSIMUStateEstimator.cpp), the estimator the field
 * node defaults to (QuadRappidsPlannerAndController/ExampleVehicleStateMachine.cpp:11, :419), for every vehicle of an
 * ensemble on the device: nine states in double with a 9x9 covariance per vehicle.  The node feeds it in three places,
 * and so does a host here:
 *     afe_gps_estimator_imu       CallbackIMU (:68-77): Predict(acc, gyro) on every IMU message -- every logic tick
 *                                 (Simulator/main.cpp:229, 500 Hz)
 *     afe_gps_estimator_measure   CallbackGPSEstimator (:79-85): UpdateWithMeasurement(pos) at 100 Hz (:228); the
 *                                 position is the engine's true one (Simulator/main.cpp:428-432 publishes the truth)
 *     an attached follower        EstGetState (:816-817): GetCurrentEstimate(), no prediction ahead;
 *                                 EstSetPredictedValues (:833-835) does nothing, so nothing is announced
 * The offboard loop is  [step to the tick -> _imu] x 5 -> _measure -> [render -> plan] -> follower tick; nothing of the
 * state or of the IMU sample leaves the device.  The sample is what the simulated vehicle's GetAccelerometer /
 * GetRateGyro return (Quadcopter_T.hpp:75-82): the logic's mount-rotated, low-passed values (QuadcopterLogic.hpp:40-52,
 * :71-77).  The gyro value is the engine's own filter output; the accelerometer goes through a filter the estimator
 * keeps (cutoff accel_lowpass_cutoff, QuadcopterLogic.cpp:102), which starts at 0 at creation: it equals the reference
 * vehicle's only if the estimator is created before the first logic tick.
 * csrc/afe_gps_estimator.hip states the arithmetic (tests/gps_imu_reference.py restates the class line by line in scalar
 * Python, tests/gps_estimator_checker.py in numpy): IEEE double, uncontracted, in a fixed order; only sin, cos and acosf
 * are the device library's.  The reference class itself is not compiled anywhere here (it needs Eigen): the restatement
 * is not pinned to it.  Times are relative to afe_time_us at creation.  Indices are engine-local.  The estimator BORROWS
 * the engine and needs one whose state is in device memory and whose rates logic is on.  Destroy order: follower,
 * estimator, engine. */
typedef struct afe_gps_estimator afe_gps_estimator;
typedef struct afe_gps_estimator_config {
  size_t struct_bytes;          /* IN: sizeof(afe_gps_estimator_config) as the caller was compiled; less is AFE_ERR_INVALID_ARG */
  double init_sigma_pos;        /* [m]     3            GPSIMUStateEstimator.cpp:21-27 */
  double init_sigma_vel;        /* [m/s]   3 */
  double init_sigma_att;        /* [rad]   10 pi / 180 */
  double sigma_acc;             /* [m/s^2] 5 */
  double sigma_gyro;            /* [rad/s] 0.1 */
  double sigma_pos;             /* [m]     0.25 */
  float accel_lowpass_cutoff;   /* [rad/s] 100          QuadcopterLogic.cpp:102 */
} afe_gps_estimator_config;
int afe_gps_estimator_default_config(afe_gps_estimator_config *cfg);   /* pure host */
/* The constructor (:9-30, Reset() once: numResets 1) for every vehicle.  AFE_ERR_NOT_CONFIGURED without
 * afe_set_rates_logic, AFE_ERR_INVALID_ARG for a host-visible engine. */
int afe_gps_estimator_create(afe_engine *e, const afe_gps_estimator_config *cfg, afe_gps_estimator **out);
int afe_gps_estimator_destroy(afe_gps_estimator *g);   /* NULL is AFE_ERR_INVALID_ARG */
/* Pure host; any pointer may be NULL.  last_tick: the afe_logic_ticks value whose sample the last _imu consumed (0: none). */
int afe_gps_estimator_info(const afe_gps_estimator *g, int64_t *n_vehicles, uint64_t *n_imu, uint64_t *n_measures, uint64_t *last_tick);
/* Predict(acc, gyro) (:66-203) for every vehicle with the sample of the latest logic tick, at afe_time_us.  Every sample
 * must be seen exactly once: AFE_ERR_NOT_CONFIGURED, with nothing changed, unless afe_logic_ticks is one more than at the
 * previous _imu (the first call needs at least one tick); afe_steps_until_tick says how far to step.  Does not wait. */
int afe_gps_estimator_imu(afe_gps_estimator *g);
/* UpdateWithMeasurement(the engine's position now) (:206-258).  n_reinitialised: the vehicles that took the singular
 * branch (:228-237) in this call; NULL: nothing is downloaded and the call does not wait.  The reference's products are
 * dense: a covariance with ANY entry that is not finite makes S non-finite and takes that branch, and is NaN everywhere
 * after a Predict (afe_gps_estimator.hip, NON-FINITE NUMBERS). */
int afe_gps_estimator_measure(afe_gps_estimator *g, int64_t *n_reinitialised);
/* Planar [comps][count]: est13 (pos 3, vel 3, att 4, ang_vel 3), cov81 (row major, all 81 words: after a Predict the
 * matrix is symmetric in value but not in bits), the times of the last Predict and of the last good update, initialized,
 * numResets.  An array that is NULL is not read back; all of them NULL is AFE_ERR_INVALID_ARG. */
int afe_gps_estimator_get_state(afe_gps_estimator *g, int64_t first, int64_t count, double *est13, double *cov81, uint64_t *last_predict_us,
                                uint64_t *last_update_us, uint8_t *initialized, uint32_t *num_resets);
/* For tests and resumption: the given arrays (NULL: left as it is; all NULL is AFE_ERR_INVALID_ARG) are written, corr3 being
 * _lastMeasUpdateAttCorrection, and the vehicles are marked initialised. */
int afe_gps_estimator_set_state(afe_gps_estimator *g, int64_t first, int64_t count, const double *est13, const double *cov81,
                                const double *corr3);
/* Reset() (:32-44) for vehicles [first, first+count) at the time of the call, and the accelerometer low-pass at 0.  Does not wait. */
int afe_gps_estimator_reset(afe_gps_estimator *g, int64_t first, int64_t count);
/* Self-test hook: the device library's functions exactly as the kernels call them, on GPU `device` (< 0: current).
 * op 0 = sin, 1 = cos (double), 2 = acosf of x narrowed to float, widened to double; x, y double [n]. */
int afe_gps_estimator_selftest_math(int device, int op, int64_t n, const double *x, double *y);
/* While a GPS estimator is attached (it must borrow the same engine, else AFE_ERR_INVALID_ARG; NULL detaches; attaching
 * one kind of estimator while the other kind is attached is AFE_ERR_INVALID_ARG), afe_follower_planner_inputs,
 * afe_follower_plan and afe_follower_tick read position, velocity and attitude from its estimate, and announce nothing.
 * Such a call is AFE_ERR_NOT_CONFIGURED unless the estimator has had an _imu at the current afe_logic_ticks. */
int afe_follower_attach_gps_estimator(afe_follower *f, afe_gps_estimator *g);

/* ---- flight stage machine -------------------------------------------------------
 * The mission of the field node for a whole ensemble, on the device: ExampleVehicleStateMachine::Run of the GPS node
 * (AIFS_ROS/hiperlab_rostools/src/QuadGPSRatesControl/ExampleVehicleStateMachine.cpp:106-379 with its main.cpp) -- wait, spool
 * the motors up, take off, fly a demonstration trajectory, land, idle, exit -- with Offboard::SafetyNet
 * (Components/Components/Offboard/SafetyNet.hpp) deciding every period whether a vehicle is killed, and the command from
 * QuadcopterController::Run (QuadcopterController.cpp:11-74): the position controller with thrust saturation, a tilt floor
 * and a commanded yaw, which the follower (RunTracking) does not cover.  Built like the follower: one lane per vehicle, planar
 * slabs of its own, the engine's stream, the engine's rates-command slabs; nothing of the state is downloaded.
 * csrc/afe_stages.hip states every value operation by operation in the reference's statement order -- the later assignment to
 * the stage wins, so an unsafe vehicle whose spool-up time has passed goes to Takeoff, not Emergency; those overrides are the
 * reference's and are kept.  tests/stage_machine_reference.py restates the three classes line by line in scalar Python,
 * tests/stages_checker.py in numpy.  The class needs ROS and Eigen headers and is compiled nowhere here: the restatement is NOT
 * pinned to the reference's binary.
 * Two writers: a follower and a stage machine on one engine both write the rates command; the last writer's stands.
 * The step kernel's logic has no sticky FS_KILLED: Emergency is never left and sends a kill every period, so the effect is the same
 * (with an onboard flight computer, afe_onboard_*, FS_KILLED and FS_PANIC are sticky, and afe_onboard_telemetry is a source for
 * afe_stages_set_warnings).
 * Not covered: the mocap node's variant of the class (the device mocap estimator keeps no last-good-measurement time and its
 * announce ring needs per-stage rules), PublishEstimate's Euler angles, delivery between ticks, rappids_headless.
 * Indices are engine-local.  The machine BORROWS the engine (and an attached estimator) and needs an engine whose state is in
 * device memory and whose rates logic is on.  Destroy order: stage machine, estimator, engine. */
enum {
  AFE_STAGE_WAIT_FOR_START = 0, AFE_STAGE_SPOOL_UP = 1, AFE_STAGE_TAKEOFF = 2, AFE_STAGE_FLIGHT = 3, AFE_STAGE_LANDING = 4,
  AFE_STAGE_COMPLETE = 5, AFE_STAGE_EMERGENCY = 6, AFE_STAGE_COUNT = 7    /* ExampleVehicleStateMachine.hpp:26-34 */
};
enum {                                    /* SafetyNet::SafetyState, one bit each */
  AFE_SAFETY_NOT_SEEN = 1, AFE_SAFETY_UNSAFE_POSITION = 2, AFE_SAFETY_UPSIDE_DOWN_AND_LOW = 4, AFE_SAFETY_USER_UNSAFE = 8
};
#define AFE_WARN_LOW_BATT 0x01            /* TelemetryPacket.hpp:22 */
typedef struct afe_stages afe_stages;
typedef struct afe_stages_config {
  size_t struct_bytes;          /* IN: sizeof(afe_stages_config) as the caller was compiled; less is AFE_ERR_INVALID_ARG */
  uint64_t period_us;           /* mainLoopFrequency = 50 Hz: 20 000 */
  uint64_t delay_us;            /* command radio delay: 30 000 */
  float nat_freq, damping;      /* as afe_follower_default_config derives the four */
  float att_time_const_xy, att_time_const_z;
  double min_corner[3];         /* SetSafeCorners, ExampleVehicleStateMachine.cpp:88: (-100, -100, -2) */
  double max_corner[3];         /* (100, 100, 20); a pair that is not ordered is AFE_ERR_INVALID_ARG (the reference asserts) */
  double min_normal_height;     /* 0 */
  double not_seen_timeout_s;    /* SafetyNet.hpp:57: 0.5 */
  double spool_up_time_s;       /* :145: 0.5 */
  double spool_up_thrust_by_weight; /* :146: 0.25 */
  double takeoff_time_s;        /* :185: 2 */
  double get_into_action_time_s;/* :222, :323: 2 */
  double landing_speed;         /* :322: 0.5 m/s */
  int traj_id;                  /* :219: 3 (0 fixed point, 1 circle, 2 SHM, 3 circle at fixed height, 4 circle with sinusoidal
                                   height and yaw, 5 yaw at a fixed position); outside 0..5 is AFE_ERR_INVALID_ARG */
} afe_stages_config;
/* The reference's constants and the controller's parameters for the type (1, 2, 4, 5; else AFE_ERR_INVALID_ARG).  Pure host. */
int afe_stages_default_config(int quadcopter_type, afe_stages_config *cfg);
/* The constructor and Initialize for every vehicle: WaitForStart with last stage Complete, vehicleNotSeen set, desired position
 * and yaw 0, the circle centre (0, -2) for traj_id 1 and (0, 0) otherwise, nothing in flight.  The ring follows
 * afe_follower_ring_slots.  AFE_ERR_NOT_CONFIGURED without afe_set_rates_logic, AFE_ERR_INVALID_ARG for a host-visible engine. */
int afe_stages_create(afe_engine *e, const afe_stages_config *cfg, afe_stages **out);
int afe_stages_destroy(afe_stages *s);   /* NULL is AFE_ERR_INVALID_ARG */
/* (any output may be NULL) ticks so far, messages in flight after the last tick */
int afe_stages_info(const afe_stages *s, int64_t *n_vehicles, int *slots, uint64_t *n_ticks, int *in_flight);
/* _desiredPosition (pos3 planar [3][count]), _desiredYawAngle (yaw [count]) and the circle centre's x and y of traj_id 1, 3, 4
 * (xy2 planar [2][count]; the reference has one constant for all, an ensemble wants one per vehicle).  NULL is
 * AFE_ERR_INVALID_ARG; count == 0 with a valid range is AFE_OK without touching the engine. */
int afe_stages_set_desired_position(afe_stages *s, int64_t first, int64_t count, const double *pos3);
int afe_stages_set_desired_yaw(afe_stages *s, int64_t first, int64_t count, const double *yaw);
int afe_stages_set_centre(afe_stages *s, int64_t first, int64_t count, const double *xy2);
/* SetExternalPanic -> SafetyNet::SetUnsafe: userUnsafe of the vehicles, for good. */
int afe_stages_set_unsafe(afe_stages *s, int64_t first, int64_t count);
/* A per-vehicle request that is OR-ed with the tick's shouldStart / shouldStop and stays until changed. */
int afe_stages_request(afe_stages *s, int64_t first, int64_t count, int start, int stop);
/* CallbackTelemetry's _lastTelWarnings, warnings [count]; HaveLowBattery() is bit AFE_WARN_LOW_BATT.  The simulated vehicle
 * never reports a low battery by itself (Quadcopter_T.cpp:72 hands the logic 1.2 x the threshold). */
int afe_stages_set_warnings(afe_stages *s, int64_t first, int64_t count, const uint8_t *warnings);
/* Run(shouldStart, shouldStop) for every vehicle at now = afe_time_us, on the engine's stream (a resident step grid ends first):
 * stage bookkeeping, state read (the engine's truth, or the attached estimator's estimate), safety net, the switch, Run, codec
 * and delay line; the newest due message becomes the engine's rates command as afe_set_commands_from_radio would leave it
 * (type 5: the four floats, have 1; idle and kill: zeros, have 0; WaitForStart's default message: nothing).  Messages are
 * delivered AT TICKS ONLY.  counts8 (may be NULL: then nothing is downloaded and the call does not wait): vehicles per stage
 * after the tick [0..6] and vehicles ready to exit [7]; GetIsReadyToExit of the ensemble is counts8[7] == n.  A tick that would
 * leave more messages in flight than the ring holds is AFE_ERR_OUT_OF_RANGE. */
int afe_stages_tick(afe_stages *s, int should_start, int should_stop, int64_t *counts8);
/* What afe_stages_get reads back, planar [comps][count]; a pointer that is NULL is not read back, all NULL is AFE_ERR_INVALID_ARG. */
typedef struct afe_stages_fields {
  size_t struct_bytes;          /* IN: sizeof(afe_stages_fields) */
  uint8_t *stage, *last_stage;  /* AFE_STAGE_* */
  uint64_t *t0_us;              /* afe_time_us at the last stage timer reset */
  uint8_t *safety;              /* AFE_SAFETY_* bits of the last tick */
  uint8_t *ready;               /* _vehicleIsReadyForProgramToExit */
  double *init_pos3, *desired_pos3, *last_pos3, *last_vel3, *last_acc3;
  double *cmd_yaw;              /* _cmdYawAngle */
  float *computed4, *sent4;     /* the last tick's command before and after the radio codec (zeros for types 0, 6, 2) */
  uint8_t *msg_type;            /* its type: 0, 5 (rates), 6 (idle), 2 (kill) */
} afe_stages_fields;
int afe_stages_get(afe_stages *s, int64_t first, int64_t count, const afe_stages_fields *fields);
/* While attached (the estimator must borrow the same engine, else AFE_ERR_INVALID_ARG; NULL detaches) a tick reads position,
 * velocity and attitude from GetCurrentEstimate() and the safety net's time since the last good measurement from the estimator.
 * Such a tick is AFE_ERR_NOT_CONFIGURED unless the estimator has had an _imu at the current afe_logic_ticks.  Without an
 * estimator that time is 0: the truth is always seen. */
int afe_stages_attach_gps_estimator(afe_stages *s, afe_gps_estimator *g);
/* Self-test hook: the device library's functions exactly as the tick kernel calls them, through the same helpers, on GPU
 * `device` (< 0: current).  op 0, 1 = sin, cos (x, y double [n]); op 2..5 = sinf, cosf, asinf, acosf (x, y float [n]). */
int afe_stages_selftest_math(int device, int op, int64_t n, const void *x, void *y);

/* ---- onboard flight computer (csrc/afe_onboard.hip) -----------------------------------------------------------------------
 * The rest of Onboard::QuadcopterLogic::Run (Components/Components/Logic/QuadcopterLogic.cpp:164-219 with what
 * Quadcopter_T.cpp:163-185 hands it) for a whole ensemble WITHOUT UWB ranging: battery, accelerometer and temperature low-passes,
 * the main-loop and command-rate monitors, the attitude estimate of KalmanFilter6DOF::Predict's complementary branch
 * (KalmanFilter6DOF.cpp:70-147 -- all the reference executes when no UWB network exists, and Rappids_Simulator builds none),
 * ParseIncomingCommunications with STICKY FS_PANIC and FS_KILLED, the five telemetry warnings, CheckPanicReasons, the
 * external-acceleration controller and the telemetry packets.  A consumer of the engine like the follower and the stage
 * machine: one lane per vehicle, planar slabs of its own, the engine's stream, one kernel per logic tick BEHIND the step that
 * fired the tick; no step kernel knows about it.  The step kernel keeps computing the rates command (one writer per value):
 * for a vehicle in FS_EXTERNAL_RATES_CONTROL the onboard tick leaves the command as it stands, in the acceleration state it
 * writes its own four motor speeds, and in IDLE, PANIC and KILLED it writes zeros OVER what the step kernel wrote.
 * csrc/afe_onboard.hip states every value operation by operation; tests/onboard_checker.py restates it in numpy.  The
 * restatement is unpinned except for the parts listed in the README (QuadcopterLogic.hpp pulls in the 9x9 Eigen filter).
 * THE CLOCK of a tick is the engine clock at the START of the step that fired it (the reference's logic reads the master clock
 * inside Quadcopter_T::Run, before main.cpp:392 advances it).  Radio arrivals carry afe_time_us at the moment of delivery.
 * THE RADIO MAILBOX: while an onboard computer exists every delivery of a command -- afe_set_rates_commands (type 5, flags 0),
 * afe_set_commands_from_radio, a follower's or stage machine's tick, afe_onboard_radio -- also records (arrival time, type,
 * flags) per vehicle.  ONE delivery per vehicle between two onboard ticks is represented: a second one overwrites the first
 * and the command-rate monitor sees one.  A delivery stamped later than the tick's clock (made between the ticking step and the
 * onboard tick) waits for the next tick -- but its floats are in the rates-command slab already, so for that one tick the
 * telemetry forces of a rates-state vehicle come from the new command and its motor command from the old one: deliver between
 * ticks.  After afe_load_checkpoint the clock of the latest tick is unknown: afe_onboard_tick is refused until the next tick has fired.
 * Without an onboard computer nothing changes for anybody.
 * NOT BUILT: UWB range updates and the 9x9 covariance, FS_FULLY_AUTONOMOUS (a position command is refused), TestMotors, gyro
 * and propeller calibration (a calibrateMotors flag is ignored).  Estimated position and velocity stay 0, as in the reference
 * without UWB, so PANIC_ONBOARD_ESTIMATE_CRAZY and PANIC_UWB_TIMEOUT cannot fire; both comparisons are kept in the code.
 * It equals the reference's vehicle only when created before the first logic tick (its filters and timers start at creation).
 * Indices are engine-local.  The computer BORROWS the engine; destroy order: onboard computer, then the engine. */
enum {                                    /* QuadcopterLogic::FlightState, QuadcopterLogic.hpp:148-157 */
  AFE_FS_UNINITIALIZED = 0, AFE_FS_IDLE = 1, AFE_FS_FULLY_AUTONOMOUS = 2, AFE_FS_PANIC = 3, AFE_FS_KILLED = 4,
  AFE_FS_EXTERNAL_ACCELERATION_CONTROL = 5, AFE_FS_EXTERNAL_RATES_CONTROL = 6, AFE_FS_COUNT = 7
};
enum {                                    /* PanicReason.hpp */
  AFE_PANIC_NO_PANIC = 0, AFE_PANIC_ONBOARD_ESTIMATE_CRAZY = 1, AFE_PANIC_UWB_TIMEOUT = 2, AFE_PANIC_UPSIDE_DOWN = 3,
  AFE_PANIC_RADIO_CMD_TIMEOUT = 4, AFE_PANIC_LOW_BATTERY = 5, AFE_PANIC_KILLED_INTERNALLY = 6, AFE_PANIC_KILLED_EXTERNALLY = 7,
  AFE_PANIC_COUNT = 8
};
#define AFE_WARN_CMD_RATE 0x02            /* TelemetryPacket.hpp:22-27 */
#define AFE_WARN_UWB_RESET 0x04
#define AFE_WARN_ONBOARD_FREQ 0x08
#define AFE_WARN_CMD_BATCH_DROP 0x10
#define AFE_RADIO_FLAG_DISABLE_SAFETY_CHECKS 0x02   /* RadioTypes::disableOnboardStateSafetyChecks */
typedef struct afe_onboard afe_onboard;
typedef struct afe_onboard_config {
  size_t struct_bytes;          /* IN: sizeof(afe_onboard_config) as the caller was compiled; less is AFE_ERR_INVALID_ARG */
  float accel_lowpass_cutoff;   /* [rad/s] 100                  QuadcopterLogic.cpp:102 */
  float batt_lowpass_cutoff;    /* [rad/s] 0.5f * float(2 pi)   :104 */
  float temp_lowpass_cutoff;    /* [rad/s] 0.5f * float(2 pi)   :105 */
  float main_loop_monitor_cutoff; /* [rad/s] 50                 :15 */
  float cmd_rate_monitor_cutoff;  /* [rad/s] 1                  :14 */
  float att_time_const_xy, att_time_const_z;   /* QuadcopterConstants attControl_timeConst_* */
  float low_battery_threshold;  /* [V] afe_low_battery_threshold_from_type; the warning is at 1.05f x this */
  float radio_cmd_period;       /* [s] 0.02                     :10 */
} afe_onboard_config;
/* The reference's values for the type (1, 2, 4, 5; else AFE_ERR_INVALID_ARG).  Pure host. */
int afe_onboard_default_config(int quadcopter_type, afe_onboard_config *cfg);
/* Initialise() for every vehicle: FS_IDLE, no panic, filters at their initial values, battery measurement 1.2f x threshold of the
 * vehicle's type, all timers reset to afe_time_us.  cfg_table: one config per type record (n_types must equal the type table's
 * size; it pairs with the logic table).  AFE_ERR_NOT_CONFIGURED without afe_set_rates_logic, AFE_ERR_INVALID_ARG for a
 * host-visible engine or an engine that has an onboard computer already. */
int afe_onboard_create(afe_engine *e, const afe_onboard_config *cfg_table, int n_types, afe_onboard **out);
int afe_onboard_destroy(afe_onboard *o);   /* withdraws the mailbox from the engine; NULL is AFE_ERR_INVALID_ARG */
/* (any output may be NULL) onboard ticks so far; the afe_logic_ticks value the last one consumed (0: none) */
int afe_onboard_info(const afe_onboard *o, int64_t *n_vehicles, uint64_t *n_ticks, uint64_t *last_tick);
/* The voltage Quadcopter_T hands SetBatteryMeasurement at every tick, volts [count].  NULL is AFE_ERR_INVALID_ARG; count == 0
 * with a valid range is AFE_OK without touching the engine. */
int afe_onboard_set_battery(afe_onboard *o, int64_t first, int64_t count, const float *volts);
/* SetCommandRadioMsg for a vehicle with an onboard computer, raw_packets [count][AFE_RADIO_PACKET_SIZE].  Types 2, 5, 6 do what
 * afe_set_commands_from_radio does; type 4 (externalAccelerationCmd) stores its four floats for the onboard controller and
 * clears the vehicle's rates command; any other type (3, the position command, needs the range filter) is
 * AFE_ERR_INVALID_ARG with nothing applied. */
int afe_onboard_radio(afe_onboard *o, int64_t first, int64_t count, const uint8_t *raw_packets);
/* One Run() for every vehicle with the IMU sample of the latest logic tick.  AFE_ERR_NOT_CONFIGURED, with nothing changed, unless
 * afe_logic_ticks is exactly one more than at the previous call (the first call: one more than at creation) and no step has run
 * after the ticking one (afe_steps_until_tick says how far to step).  counts16 (may be NULL: then nothing is
 * downloaded and the call does not wait): vehicles per flight state after the tick [0..6], per first panic reason [7..14], and
 * vehicles with any warning bit accumulated [15]. */
int afe_onboard_tick(afe_onboard *o, int64_t *counts16);
/* What afe_onboard_get reads back, planar [comps][count]; a pointer that is NULL is not read back, all NULL is AFE_ERR_INVALID_ARG. */
typedef struct afe_onboard_fields {
  size_t struct_bytes;          /* IN: sizeof(afe_onboard_fields) */
  uint8_t *flight_state;        /* AFE_FS_* */
  uint8_t *panic_reason;        /* _firstPanicReason, AFE_PANIC_* */
  uint8_t *warnings;            /* _telWarnings: accumulated since the last telemetry */
  float *est_att4, *est_ang_vel3;   /* GetEstimate (position and velocity are 0) */
  float *acc_filtered3;         /* _imuAccelerometer.lowPass.GetValue() */
  float *batt_filtered;         /* _battMeas.voltageFiltered */
  float *main_loop_dt, *cmd_dt; /* the two MonitorSimplePeriod::lpDt */
  float *motor_forces4;         /* _desMotorForcesForTelemetry */
  uint32_t *cycle_counter;
  uint64_t *last_radio_us;      /* afe_time_us at the last SetRadioMessage (creation time: none yet) */
  uint8_t *motors_running;      /* GetAreMotorsRunning() after the last tick */
} afe_onboard_fields;
int afe_onboard_get(afe_onboard *o, int64_t first, int64_t count, const afe_onboard_fields *fields);
/* For tests and resumption, planar [comps][count]; NULL leaves a field as it is, all NULL is AFE_ERR_INVALID_ARG.  lowpass20:
 * xm0, xm1, ym0, ym1 of the accelerometer (3 each, 12 rows), then of the battery (4 rows) and the temperature (4 rows). */
typedef struct afe_onboard_state {
  size_t struct_bytes;          /* IN: sizeof(afe_onboard_state) */
  const float *est_att4, *est_ang_vel3;
  const uint8_t *imu_initialized;   /* KalmanFilter6DOF::_IMUInitialized: 0 makes the next tick rebuild the attitude */
  const float *lowpass20;
  const uint8_t *flight_state;
  const uint8_t *motors_running;
  const uint64_t *last_radio_us;
} afe_onboard_state;
int afe_onboard_set_state(afe_onboard *o, int64_t first, int64_t count, const afe_onboard_state *state);
/* GetTelemetryDataPackets (QuadcopterLogic.cpp:621-679): packets [count][2][AFE_TELEMETRY_PACKET_SIZE], both parts per vehicle
 * (bytes the reference leaves unwritten are 0).  Afterwards the packet counter of the vehicles IN THE RANGE is incremented and
 * their warnings are cleared. */
int afe_onboard_telemetry(afe_onboard *o, int64_t first, int64_t count, uint8_t *packets);
/* Self-test hook: the device library's functions exactly as the tick kernel calls them, through the same helpers, on GPU
 * `device` (< 0: current).  op 0..3 = sinf, cosf, acosf, asinf (x, y float [n]); op 4 = atan2f (x float [2][n]: y then x). */
int afe_onboard_selftest_math(int device, int op, int64_t n, const float *x, float *y);

/* ---- stepping -----------------------------------------------------------
 * afe_step replaces the loop body
 *     for (v : vehicles) v->Run();  simTimer.AdvanceMicroSeconds(dt_us);
 * (Simulator/Rappids_Simulator/main.cpp:391-392; AIFS_ROS/.../Simulator/
 * main.cpp:323-325) n_steps times: every vehicle takes n_steps physics steps
 * of dt = dt_us * 1e-6 s (Quadcopter_T.cpp:85-156, Motor.cpp:39-84).  The
 * engine clock advances by dt_us per step; whenever the onboard-logic gate of
 * Quadcopter_T.cpp:159-160 fires (strict >, then minus one period) the step
 * also synthesises the IMU sample of :165-180 into the IMU buffers and counts
 * one logic tick.  dt_us == 0 is the reference's "dt < 1e-6: return".
 * Within one call the motor commands and external wrench are held constant,
 * as they are between two logicType::Run() calls in the reference.
 * afe_steps_until_tick tells a host-side logicType driver how many steps of
 * dt_us may be fused before its Run() is due (>= 1). */
int afe_step(afe_engine *e, uint64_t dt_us, int n_steps);
/* How the step kernels address the state slabs: 0 (default) -- through buffer resources spanning the engine's
 * arenas whenever those fit 32-bit offsets (up to ~31 M fp32 vehicles), otherwise by global addresses; 1 -- always by
 * global addresses.  Same results bit for bit; mode 1 exists so that the kernels very large ensembles run are
 * testable at any size. */
int afe_set_addressing(afe_engine *e, int mode);
/* Which step kernel the next afe_step will launch: record_path 0 = parameters in the kernel arguments (all
 * vehicles on record 0), 1 = one scalar-loaded record per wave (type constant over every aligned run of 64),
 * 2 = type table in LDS; addressing 0 = buffer resources, 1 = global addresses.  Either pointer may be NULL. */
int afe_step_kernel_info(const afe_engine *e, int *record_path, int *addressing);

/* Split stepping.  With two parts afe_step launches the first half of the ensemble on the engine's stream and the
 * second half on a stream of its own, and the two chains of launches never wait for each other -- each one's
 * drain-and-dispatch gap (a fixed ~2.7 us per launch) is covered by the other's streaming.  At 2^20 vehicles a
 * 1 ms step takes 22.1 instead of 24.4 us; per-vehicle results are the same bits (vehicles do not interact).
 * What changes is WHEN the engine's stream is ordered after the steps: not at the return of afe_step but at the
 * next engine call that touches device state or the stream (afe_sync, getters and setters, afe_event_record,
 * afe_pack_positions, the queries, the depth camera, checkpoints, ... every entry point but afe_step joins the
 * two streams first).  While the engine uses its OWN stream nobody else can queue work on it, so the difference
 * cannot be observed.
 *   parts = 0 (default): automatic -- two parts for ensembles of 2^19 vehicles and more as long as the engine owns
 *     its stream; one launch on one stream otherwise (smaller ensembles lose: the second launch costs more host
 *     time than it hides; a caller-owned stream keeps the order-at-return behaviour).
 *     (Engines an afe_group creates for several devices start with parts = 1: one host thread launches for all of
 *     them, and a second launch per shard and step would make that thread the limit.)
 *   parts = 1: never.   parts = 2: always (ensembles of 1 024 vehicles and more), also on a caller-owned stream
 *     (afe_set_stream) -- a host that queues its own work there and expects it to see the stepped state must
 *     then call afe_sync or afe_event_record in between. */
int afe_set_split_stepping(afe_engine *e, int parts);

/* Key of the counter-based noise generator (AFE_SEED_COUNTER); default 0. */
int afe_set_noise_seed(afe_engine *e, uint64_t seed);

/* BASELINE config 4's disturbance process on the device: a per-vehicle wind-gust force through the SetExternalForce
 * port (Components/Components/Simulation/Quadcopter_T.hpp:45, applied at Quadcopter_T.cpp:132; the reference has the
 * port and no model behind it).  While enabled the engine owns the external-force slab: during epoch
 * k = floor(step start time / period_us) vehicle i feels F = sigma_i (z0, z1, z2) with sigma_i = sigma_max * g / (n_global - 1),
 * g = first_global_index + i, and z = N(0,1) from the counter-based generator at (seed, g, epoch k) -- piecewise
 * constant, resampled on the device when a step starts in a new epoch ("N(0, sigma^2), sigma swept
 * 0...0.5 N, piecewise-constant 100 ms").  No host upload, no per-step cost; the force of (vehicle, epoch) does not
 * depend on sharding or on how the steps are issued.  n_global <= 0: this ensemble alone.  enabled = 0 leaves the
 * slab as it is (afe_set_external_force takes over).  afe_get_external_force reads the slab back. */
int afe_set_gust_process(afe_engine *e, int enabled, uint64_t seed, double sigma_max, uint64_t period_us, int64_t n_global);
int afe_get_external_force(afe_engine *e, int64_t first, int64_t count, double *force3);

/* Persistent stepping: afe_step without a kernel launch per step.  The step loop of the reference
 * (`for each vehicle: Run(); clock += dt`, Simulator/Rappids_Simulator/main.cpp:330,391-392;
 * AIFS_ROS/hiperlab_rostools/src/Simulator/main.cpp:323-325) has no barrier between vehicles, so nothing in it
 * asks for one between two steps of different vehicles either.  In this mode ONE resident grid of one-wave
 * workgroups stays on the device; afe_step(e, dt, k) authorises k more steps by writing k 8-byte descriptors
 * (step number, logic-tick flag) into a ring in pinned host memory and returns; every wave advances ITS vehicles
 * through each descriptor as it appears -- loads, the step, stores: the body of the one-step launch, the state
 * back in HBM after every step, bit for bit the launched kernels' results.  What a dependent launch costs on top
 * of its streaming time (2.7 us here: drain, dispatch, ramp-up) is not paid; an ensemble of 131 072 vehicles --
 * one GPU's shard of the 1 M-vehicle configuration on eight -- steps in [see DESIGN.md section 6] instead of 5.6 us.
 * The grid leaves the device ("parks") when any other entry point needs the stream or the state (afe_sync, getters,
 * setters, events, queries, checkpoints ...: they all do it implicitly and the next afe_step starts a new grid), and
 * by itself when the host has not authorised a step for ~200 us, so nothing -- not even a device-wide
 * synchronisation issued elsewhere -- can wait on it for ever.  A grid of a large ensemble occupies every wave slot of
 * the device while it is resident: another engine's grid, or any other kernel of the process, starts when it has left
 * (two such engines stepped alternately take turns, each handing over after its 200 us of idling -- correct, slow:
 * tests/test_gpu_persistent.py; one process, one large resident grid per device is the intended use).  A grid that starts
 * while another engine's launch is running may find the register file fragmented and a few of its workgroups without a
 * slot; the grid notices (60 ms), parks at one step and is started again -- results are unaffected, stderr says so.
 *   mode = AFE_STEP_LAUNCH (0, default): one kernel launch per step (or per afe_set_max_fused_steps chunk).
 *   mode = AFE_STEP_PERSISTENT (1): as above, whenever the ensemble qualifies -- every vehicle on type record 0,
 *     no external torque, the engine's own stream, an arena below 4 GiB; otherwise the launches, silently.
 *   mode = AFE_STEP_AUTO (2): the engine picks per call.  One step per call: the resident grid in its resident-state
 *     form (AFE_STEP_RESIDENT below: the same bits, fewer bytes) for ensembles of up to 2^20 vehicles, launches (split,
 *     see above; cache-policy hints by size, afe_set_cache_policy) beyond.  Several steps per call (nothing is observable in between): from
 *     8 steps, or from 2 at 2^19 vehicles and more, fused launches -- the state stays in registers from step to step --
 *     which is the fastest way to the same bits there (measured table: DESIGN.md section 6).
 * afe_steps_completed: the number of steps (since afe_create) that EVERY vehicle has been advanced through -- the
 * per-step completion word of the resident grid, readable at any time without disturbing it; in launch mode the
 * number of steps issued.  (Reading the state itself goes through the getters, which park the grid first.) */
#define AFE_STEP_LAUNCH 0
#define AFE_STEP_PERSISTENT 1
#define AFE_STEP_AUTO 2
/*   mode = AFE_STEP_RESIDENT (3): the resident grid with the steps that are ALREADY authorised taken together: a wave
 *     that finds k steps waiting loads its vehicles' inputs once, keeps the state in registers from step to step and
 *     stores each step's state as it is made -- every step still lands in memory (a host that authorises one step at a
 *     time and watches afe_steps_completed sees exactly the persistent mode), but a host that runs ahead pays for the
 *     stores only (~64 instead of ~143 bytes per vehicle-step).  Same bits.  Not what bench.py's headline measures
 *     (that one reads the state back every step); reported beside it. */
#define AFE_STEP_RESIDENT 3
int afe_set_step_mode(afe_engine *e, int mode);
int afe_steps_completed(afe_engine *e, uint64_t *steps);
/* 1 while a resident grid is on the device, 0 otherwise (diagnostic; tests use it) */
int afe_persistent_running(const afe_engine *e, int *running);
/* Device time spent by the resident grids since the last call (begin / end timestamps of each grid's dispatch on the
 * engine's own queue) and the steps they served: what rocprofv3 --kernel-trace reports as the kernel's duration,
 * measured in the run.  Ends the grid now resident (it is counted).  Both 0 when the grids ran on the HIP stream
 * (AFE_PERSIST_AQL=0, a caller's stream): use afe_event_record there.  Replaces nothing in the reference. */
int afe_grid_time(afe_engine *e, uint64_t *device_ns, uint64_t *steps);
/* Where the resident grid is dispatched: 1 = a user-mode queue of the engine's own (the grid survives afe_sync, no HIP
 * synchronisation of the process waits for it; a dispatch costs the host 14 us), 0 = the engine's HIP stream (every
 * afe_sync ends the grid, a launch costs 3 us, workers that are done leave), -1 = automatic (default): the own queue up to
 * 262 144 vehicles, where it is faster and the grid leaves a third of the wave slots to others; the HIP stream beyond
 * (at 524 288 the own queue is 5 % faster in 20-step blocks but the grid fills the device: DESIGN.md section 6).
 * Same bits either way.  Ends the grid now resident.  Replaces nothing in the reference. */
int afe_set_resident_queue(afe_engine *e, int mode);

/* Cache-policy hints of the one-step launches' slab accesses (`nt` bits on the buffer instructions; never a different
 * result bit).  -1 automatic (default): by what the 256 MiB Infinity Cache can keep from one step to the next --
 * everything (up to ~2^20 fp32 vehicles): default policy; only the state (up to ~4 M): inputs (commands, wrench) and
 * outputs (IMU samples) are streamed past it; not even the state: everything is streamed, one contiguous range per XCD.
 * 0 / 1 / 2 / 3 force one of these.  Replaces nothing in the reference (a CPU's caches decide for themselves). */
int afe_set_cache_policy(afe_engine *e, int policy);
/* the policy (0..3) the next one-step launch of this engine would carry: the forced one, or what the automatic rule
 * resolves to for the engine's size and configuration (diagnostic; tests use it) */
int afe_cache_policy_in_use(const afe_engine *e, int *policy);

/* How many sub-steps afe_step may fuse into one kernel launch (1..64, default
 * 64).  1 = one launch per step (state goes through HBM every step: the
 * per-step-observable mode bench.py reports); results are bitwise identical
 * for every setting. */
int afe_set_max_fused_steps(afe_engine *e, int max_steps_per_launch);
int afe_steps_until_tick(const afe_engine *e, uint64_t dt_us, int *n_steps);
int afe_sync(afe_engine *e);
int afe_time_us(const afe_engine *e, uint64_t *now_us);
int afe_logic_ticks(const afe_engine *e, uint64_t *n_ticks);

/* The IMU sample handed to logicType::SetIMUMeasurementRateGyro /
 * SetIMUMeasurementAccelerometer at the most recent logic tick
 * (Quadcopter_T.cpp:171,180); floats, like the reference's Vec3f. */
int afe_get_imu(afe_engine *e, int64_t first, int64_t count, float *gyro3, float *acc3);

/* ---- checkpoint / resume -------------------------------------------------
 * The reference has none (its motor speeds, timers, RNG and logic state have no
 * accessor).  Here the SoA slabs ARE the checkpoint: state,
 * motor speeds and commands, wrench, last IMU sample, RNG words, on-device logic
 * state and the engine clock.  afe_checkpoint_size gives the byte count for the
 * current configuration.  A checkpoint loads into any engine (the one that saved
 * it or a freshly created one) with the same n_vehicles / precision that has been
 * given the same type table and on-device logic table: both are fingerprinted in
 * the header and a mismatch is refused (AFE_ERR_INVALID_ARG).  The per-vehicle
 * type indices, noise switch, sigmas, seed policy, logic period, wrench flags and
 * the clock are restored from the checkpoint. */
int afe_checkpoint_size(const afe_engine *e, uint64_t *bytes);
int afe_save_checkpoint(afe_engine *e, void *host_buffer, uint64_t bytes);
int afe_load_checkpoint(afe_engine *e, const void *host_buffer, uint64_t bytes);

/* Pure host helper (no GPU): the logic-gate pattern of n_steps steps of dt_us
 * starting from *elapsed_us (time since the gate last fired), per Timer.hpp:
 * 27-54.  tick_out[i] = 1 if step i fires.  Updates *elapsed_us. */
int afe_plan_ticks(double logic_period_s, uint64_t *elapsed_us, uint64_t dt_us,
                   int n_steps, uint8_t *tick_out);

/* ---- zero-copy device view ---------------------------------------------
 * Raw device pointers to the SoA slabs for HIP-side consumers (renderers,
 * planners, torch via __cuda_array_interface__).  Each field is planar with
 * `stride` elements between components.  state_elem_size is 4 or 8.
 * motor_speed is current as of this call: for stateless motors (tau_m = J_m =
 * 0) driven by held commands the step kernel does not store the rotor speeds
 * (they are clamp(max(0, cmd))); ask for the view again, or use afe_get_state,
 * after further steps.
 * The caller sets struct_bytes = sizeof(afe_device_view) BEFORE the call: the
 * engine fills the members that fit and nothing beyond (a host compiled against
 * an older, shorter struct keeps working); less than the members up to
 * type_index is AFE_ERR_INVALID_ARG.  The call ends a resident step grid first
 * (afe_set_step_mode) and leaves the engine's stream with every authorised
 * step queued before anything the caller orders behind it: slabs read by the
 * caller's own kernels after a stream-ordered wait (or after afe_sync) hold the
 * state after the last afe_step. */
typedef struct afe_device_view {
  size_t struct_bytes;   /* IN: sizeof(afe_device_view) as the caller was compiled */
  int64_t n_vehicles;
  int64_t stride;
  int state_elem_size;
  void *pos, *vel, *att, *ang_vel, *motor_speed; /* 3,3,4,3,4 components */
  void *ext_force, *ext_torque;                  /* 3,3 components */
  float *motor_cmd;                              /* 4 components */
  float *gyro, *acc;                             /* 3,3 components */
  uint32_t *rng;
  uint8_t *type_index;   /* READ ONLY: the engine chooses its step kernel from a host mirror of this
                          * slab (afe_set_vehicle_types keeps both in step); writing it through this
                          * pointer desynchronises them */
  /* pos holds x and y RELATIVE to where they were last set (SetPosition): absolute x = pos_anchor_xy[i] + pos[i],
   * absolute y = pos_anchor_xy[stride + i] + pos[stride + i], added in double; z is absolute.  An fp32 x far from
   * the origin cannot resolve a slow vehicle's motion (at 4 km one ulp is 0.24 mm), an offset from the set point
   * can.  AFE_F64 engines keep absolute positions like the reference: their anchors are zero.  The getters,
   * afe_pack_positions and the depth camera add the anchors themselves. */
  const double *pos_anchor_xy; /* 2 components */
} afe_device_view;
int afe_get_device_view(afe_engine *e, afe_device_view *out);

/* Algorithmic HBM bytes one vehicle-step of the current configuration moves:
 * the slab accesses the step kernel actually makes (SURVEY 8d's 176 B for fp32
 * state + cmds + IMU, minus the rotor-speed read / store the configuration
 * lets it skip, +12 per active wrench array, IMU / RNG / logic bytes on a tick;
 * DESIGN.md section 3); what bench.py's roofline is computed from. */
int afe_algorithmic_bytes_per_step(const afe_engine *e, int imu_tick, double *bytes);

/* Self-test hook for the IMU noise generator: for each of n minstd_rand0 words
 * the first six std::normal_distribution<double>(0,1) draws the engine's
 * device code produces from it (normals6[6*i .. 6*i+5], libstdc++ order) and
 * the engine word afterwards.  Lets a host check the device generator against
 * libstdc++ known answers (tests/golden/rng_kat.json) without going through a
 * physics step.  Replaces nothing in the reference. */
int afe_selftest_normals(afe_engine *e, const uint32_t *seeds, int64_t n,
                         double *normals6, uint32_t *state_after);
/* The same for the AFE_F32 engine's generator: identical engine words and accepted
 * candidates; the polar multiplier and the final product are evaluated in float (the
 * sample is narrowed to float in the reference as well, Quadcopter_T.cpp:167-169),
 * each value within a few float ulp of float(libstdc++'s double). */
int afe_selftest_normals_f32(afe_engine *e, const uint32_t *seeds, int64_t n,
                             float *normals6, uint32_t *state_after);

/* ---- HIP-event timing on the engine's stream (for bench.py) ------------- */
int afe_event_create(void **event);
int afe_event_destroy(void *event);
int afe_event_record(afe_engine *e, void *event);
int afe_event_elapsed_ms(void *start, void *stop, float *ms);

/* ---- multi-GPU shared-world exchange ------------------------------------
 * The step reads no other vehicle (Quadcopter_T.cpp:85-203), so shards step with
 * no data-path collective.  The only inter-vehicle exchange of the path is the
 * shared-world query -- the reference's analogue is UWBNetwork::Run reading other
 * vehicles' true positions (Components/Components/Simulation/UWBNetwork.cpp:
 * 54-84) -- and its payload is the positions, 12 B per vehicle, gathered onto
 * every GPU at query cadence (<= 100 Hz), never per step.
 *
 * afe_pack_positions writes this shard's positions as fp32 planar xyz into a
 * caller-provided DEVICE buffer of 3*n_vehicles floats, on the engine's stream
 * (for hosts that bring their own collective, e.g. torch.distributed). */
int afe_pack_positions(afe_engine *e, float *device_xyz);

/* One process per GPU: afe_comm wraps an RCCL communicator (RCCL is loaded at
 * run time; AFE_ERR_COMM when it is absent).  Rank 0 makes the id, the host
 * hands it to the other ranks by whatever means it has (MPI, a file, a socket,
 * torch.distributed), every rank calls afe_comm_create -- collectively, like
 * ncclCommInitRank. */
typedef struct afe_comm afe_comm;
#define AFE_COMM_ID_BYTES 128
int afe_comm_unique_id(uint8_t id[AFE_COMM_ID_BYTES]);
int afe_comm_create(afe_comm **out, const uint8_t id[AFE_COMM_ID_BYTES], int rank, int n_ranks, int device);
int afe_comm_info(const afe_comm *c, int *rank, int *n_ranks); /* as the communicator reports them */
int afe_comm_destroy(afe_comm *c);
const char *afe_comm_last_error(const afe_comm *c);
/* The all-gather: pack + ncclAllGather (per component, one group) on the engine's
 * stream.  counts[r] = vehicles of rank r, or NULL when every rank holds as many
 * as this one.  dev_xyz_all: DEVICE buffer of 3*n_all floats, planar [3][n_all],
 * vehicles in global order (rank 0's block first).  Asynchronous like afe_step. */
int afe_gather_positions(afe_engine *e, afe_comm *c, const int64_t *counts, float *dev_xyz_all);
/* The exchange behind it with the transport as an argument: which block goes where (counts, offsets; one all-gather per
 * component for equal shards, one broadcast per rank and component for unequal ones), over opaque buffers.  A host that
 * brings its own collective (MPI, torch.distributed) passes it here -- packed_xyz is this rank's [3][n_local] block as
 * afe_pack_positions wrote it, xyz_all the [3][n_all] result, both in whatever memory the transport moves; the
 * callbacks return 0 on success.  afe_gather_positions is this routine with RCCL on device memory; the CPU test suite
 * runs it over gloo on host memory (tests/test_sharding_gloo.py).  Pure host code: usable without a GPU. */
typedef struct afe_gather_transport {
  void *ctx;
  int (*all_gather)(void *ctx, const float *send, float *recv, int64_t count);            /* recv holds n_ranks x count */
  int (*broadcast)(void *ctx, const float *send, float *recv, int64_t count, int root);  /* root's send into everybody's recv */
  int (*group_start)(void *ctx);                                                          /* optional (NULL) */
  int (*group_end)(void *ctx);
} afe_gather_transport;
int afe_gather_exchange(const afe_gather_transport *t, int rank, int n_ranks, const int64_t *counts, int64_t n_local,
                        const float *packed_xyz, float *xyz_all);

/* One process, several GPUs -- the reference's own process model, one loop over a
 * std::vector of vehicles (AIFS_ROS/hiperlab_rostools/src/Simulator/main.cpp:
 * 58-95,323-325): the ensemble is cut into contiguous shards, shard i lives on
 * devices[i] (a device may be listed more than once: logical shards), each with
 * its own engine, stream and RNG words; first_global_index is set so that seeds
 * and neighbour indices are those of the unsharded ensemble.  Results are bit-
 * identical to one engine holding all vehicles. */
typedef struct afe_group afe_group;
int afe_group_create(afe_group **out, int64_t n_vehicles, int precision, const int *devices, int n_devices);
int afe_group_destroy(afe_group *g);
int afe_group_size(const afe_group *g, int *n_shards, int64_t *n_vehicles);
/* shard -> its engine (configure / fill / read it with the afe_* calls above) and global range */
int afe_group_shard(afe_group *g, int shard, afe_engine **engine, int64_t *first, int64_t *count);
int afe_group_step(afe_group *g, uint64_t dt_us, int n_steps); /* afe_step on every shard; launches overlap */
int afe_group_sync(afe_group *g);
/* every shard's positions onto every shard's device by direct peer copies (xGMI):
 * dev_xyz_all_out[i] (optional) = shard i's planar [3][n_vehicles] buffer, owned by the group */
int afe_group_gather_positions(afe_group *g, float **dev_xyz_all_out);
const char *afe_group_last_error(const afe_group *g);
/* *all_pairs = 1 if every pair of the group's devices has direct peer access; 0 if some pair has none
 * (IOMMU, VMs, restricted containers): such a group still works -- its gather then copies row by row with
 * hipMemcpyPeerAsync, which the runtime stages through host memory where it must -- afe_group_create says so once on
 * stderr and the gather is slower.  UNVERIFIED on a machine whose devices really lack peer access (none was available):
 * the staged path itself runs in the test suite, between peers and between logical shards of one device.  (The
 * reference's analogue is one address space for all vehicles: nothing to ask.) */
int afe_group_peer_access(const afe_group *g, int *all_pairs);
/* staged != 0: the gather uses the staged path (above) even between peers -- for a host that knows its direct copies
 * misbehave; 0: back to direct copies (refused with AFE_ERR_INVALID_ARG when a pair has no peer access). */
int afe_group_set_staged_copies(afe_group *g, int staged);

/* ---- shared-world consumers of the gathered buffer -----------------------
 * Nearest neighbour (collision / separation monitoring): for each local vehicle
 * the squared distance (fp32: ((dx*dx + dy*dy) + dz*dz), each operation rounded)
 * to, and global index of, its nearest other vehicle among all_xyz (device, fp32
 * planar, n_all vehicles); the lowest index wins among equally near ones; -1 /
 * 3.4e38 when there is none or the vehicle's own position is not finite.
 * Outputs are DEVICE buffers of n_vehicles entries.  Implementation: uniform
 * grid (counting sort by cell on the device, 3x3x3 search, further rings until
 * no unvisited cell can be closer, isolated vehicles by brute force) -- exact.
 * An engine that is a shard (n_vehicles < n_all) shapes the grid on its own block
 * of all_xyz and sorts only the other shards' vehicles near it; the cost of a query
 * then follows the shard, not the gathered ensemble.  Results do not depend on it.
 * cell_size <= 0 (and afe_nearest_neighbour): chosen from the occupied box,
 * about two vehicles per cell. */
int afe_nearest_neighbour(afe_engine *e, const float *all_xyz, int64_t n_all,
                          float *dist2_out, int32_t *index_out);
int afe_nearest_neighbour_grid(afe_engine *e, const float *all_xyz, int64_t n_all, float cell_size,
                               float *dist2_out, int32_t *index_out);
/* The same query (automatic cell size) without stalling the steps: it runs on a stream of its own, ordered behind what
 * the engine's stream holds at the call (the gather that filled all_xyz), while later afe_step calls proceed.  Whatever
 * would rewrite the gathered buffer or the query's scratch (afe_gather_positions, afe_pack_positions, another query) is
 * ordered behind it on the device; the host joins with afe_query_sync before it reads dist2_out / index_out.
 * (Measured, DESIGN.md section 5: the query and the steps both live on the memory system, so running them together
 * hides the query's launch gaps, not its traffic.) */
int afe_nearest_neighbour_async(afe_engine *e, const float *all_xyz, int64_t n_all, float *dist2_out, int32_t *index_out);
int afe_query_sync(afe_engine *e);
/* How often the grid is re-shaped from the ensemble's current bounds and spread: every
 * `every_n_queries` queries (default 1).  Re-shaping needs one 6 KB read-back, i.e. it synchronises
 * the stream; in between, queries are fully asynchronous.  Results do not depend on it (the query is
 * exact for any grid; vehicles that have left the grid's core are clamped into its boundary cells). */
int afe_set_neighbour_grid_refresh(afe_engine *e, int every_n_queries);
/* How often the vehicles are sorted into the grid's cells: every `every_n_queries` queries (default 1).  In between a
 * query keeps the cell ORDER of the last sort and only refreshes the positions in it (one pass instead of the five of a
 * counting sort); the device keeps a bound on how far any vehicle has moved since the sort and the search stops a ring
 * only where that bound allows -- the answers are exactly the sorted query's whatever the vehicles did (vehicles moving
 * centimetres between queries through cells metres wide cost nothing; an ensemble that has moved by cells searches wider
 * rings, and one that has jumped is answered by the brute force until the next sort).  A grid re-shape sorts anyway. */
int afe_set_neighbour_sort_reuse(afe_engine *e, int every_n_queries);
/* shape of the grid the last query used, and how many of its queries fell through to brute force
 * (isolated vehicles; reading that count synchronises the device).  Any pointer may be NULL. */
int afe_neighbour_grid_info(const afe_engine *e, int dims[3], float *cell_size, int64_t *n_cells, int64_t *n_bruteforce);
/* The O(n_queries * n_all) definition itself, for listed local vehicles (DEVICE
 * array of local indices): the cross-check of the grid at full ensemble size.
 * dist2_out / index_out are indexed by local vehicle like above. */
int afe_nearest_neighbour_bruteforce(afe_engine *e, const float *all_xyz, int64_t n_all, const int32_t *dev_queries,
                                     int64_t n_queries, float *dist2_out, int32_t *index_out);

/* Measurement aid (bench.py's `roofline.peak_measured`; SURVEY 8d asks for the box's measured streaming figure next
 * to the nominal peak): `launches` back-to-back launches of a kernel in the step kernel's own launch shape -- one-wave
 * workgroups, one lane per element, n_read planar dword read streams and n_write write streams in place through one
 * buffer resource, slab stride 256 x odd, no arithmetic to speak of -- on a scratch buffer of its own; returns the
 * best of three event-timed runs.  (n_read, n_write) = (20, 13): the 132 bytes of the off-tick step launch,
 * (24, 17): the 164 bytes of the tick launch.  No reference counterpart. */
int afe_stream_probe(int device, int64_t n, int n_read, int n_write, int launches, float *us_per_launch);

/* UWB ranging network: Simulation::UWBNetwork (Components/Components/Simulation/
 * UWBNetwork.hpp:16-50, UWBNetwork.cpp:8-89).  afe_uwb_create = the constructor's
 * rng.seed(0) (:19); afe_uwb_set_noise = SetNoiseProperties (UWBNetwork.hpp:28-33).
 * afe_uwb_range completes n_pairs ranging transactions in order, each exactly as
 * Run() does (:66-71): one uniform draw decides outlier or not, one normal draw
 * gives the noise, range = float(|p_requester - p_responder| + noise) or
 * float(normal * outlierStdDev) -- same generator and distribution classes
 * (std::mt19937, uniform_real_distribution, normal_distribution incl. its cached
 * second value), one stream for the network's lifetime (the reference's are file-scope objects shared by every
 * UWBNetwork of the process, UWBNetwork.cpp:4-6: the first network of a process matches it draw for draw; a process
 * with several networks is reproduced by drawing for all of them from ONE afe_uwb_network).  The true positions come
 * from the gathered buffer (requester / responder are GLOBAL vehicle indices, host
 * arrays); the norm is evaluated in double like Vec3d::GetNorm2.  range_out
 * (host, n_pairs floats) is what every radio "hears" (:77-80); outlier_out is
 * optional.  afe_uwb_draw exposes the stream alone (host only, no GPU). */
typedef struct afe_uwb_network afe_uwb_network;
int afe_uwb_create(afe_uwb_network **out);
void afe_uwb_destroy(afe_uwb_network *u);
int afe_uwb_set_noise(afe_uwb_network *u, double noise_std_dev, double outlier_probability, double outlier_std_dev);
int afe_uwb_draw(afe_uwb_network *u, int64_t n_pairs, double *noise_term, uint8_t *is_outlier);
int afe_uwb_range(afe_uwb_network *u, afe_engine *e, const float *dev_all_xyz, int64_t n_all,
                  const int32_t *requester, const int32_t *responder, int64_t n_pairs, float *range_out,
                  uint8_t *outlier_out);

#ifdef __cplusplus
}
#endif
#endif /* AGRIFLY_ENGINE_H */
