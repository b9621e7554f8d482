"""Talking to oracle/_ref/onboard_probe, the reference's own Onboard::QuadcopterLogic compiled where it lies (test infrastructure;
the protocol is written at the head of oracle/ref_onboard_probe.cpp).  Nothing here computes a number of the logic.

  call_lists(afa, rec)          the recorded flight (tests/onboard_flight.fly_device or synthetic_record) as one call list per
                                vehicle: tests/onboard_flight.drive_scalar -- the driver that feeds tests/onboard_reference.py --
                                with a Recorder in the place of the scalar Vehicle, so the reference receives call for call what
                                the restatement receives
  fly_reference(afa, rec)       ... through the probe -> (fields [ticks][name] like tests/onboard_checker.Onboard.fields() plus
                                est_pos, est_vel, motor_cmd; telemetry {(tick, first, count): uint8 [count, 2, 30]}; digest of
                                the request's bytes)
  vehicle_lines(afa, types)     the probe's vehicle mode: Simulation::Quadcopter_T<Onboard::QuadcopterLogic> for 20 logic ticks
  restated_vehicle_lines(...)   the same lines from tests/onboard_reference.py's TickGate and Vehicle

FROM THE ENGINE'S MAILBOX TO REFERENCE CALLS (the mapping the pin rests on):
  * a delivery (afe_set_rates_commands, afe_onboard_radio, afe_set_commands_from_radio) made at engine clock `now` is CLOCK(now),
    SetRadioMessage(type, flags, floats[0..3]) -- the radio timer and the command-rate monitor read `now`; the engine keeps ONE
    mailbox slot per vehicle between two onboard ticks, and the script delivers at most once per vehicle between two ticks, so
    nothing is lost in the mapping (a second delivery would be two SetRadioMessage calls here and one on the device:
    DESIGN 4m, not pinned);
  * a delivery stamped later than the tick's clock T (made between the ticking step and the onboard tick) goes in BEHIND that
    tick's Run, at its own clock: the device's tick leaves it in the mailbox ("msg_waits") and the next tick takes it;
  * an onboard tick at clock T is CLOCK(T), SetBatteryMeasurement(volts, -1), SetIMUMeasurementRateGyro,
    SetIMUMeasurementAccelerometer (the engine's raw samples, bit patterns), SetIMUMeasurementTemperature(25), Run -- the order
    of Quadcopter_T.cpp:163-185; afe_onboard_set_battery changes `volts` from the next tick on;
  * afe_onboard_set_state is PLACE (members written directly), afe_onboard_telemetry is GetTelemetryDataPackets behind the Run;
  * the type record with a tilted IMU mount is Initialise(type) followed by MOUNT: _IMU_* and _R rebuilt by the call Initialise
    makes; every other constant is the reference's own QuadcopterConstants(type)."""
import hashlib
import os
import struct
import subprocess

import numpy as np

from tests import onboard_checker as oc
from tests import onboard_flight as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "oracle", "_ref", "onboard_probe")
MAGIC = 0x31424f52
CLOCK, INIT, BATTERY, GYRO, ACC, TEMP, RADIO, RUN, TELEMETRY, PLACE, MOUNT = range(1, 12)
F = np.float32

# the 31 floats of a RUN record, in the probe's order -> (name, components)
FLOATS = (("est_att", 4), ("est_ang_vel", 3), ("est_pos", 3), ("est_vel", 3), ("acc_filtered", 3), ("gyro_filtered", 3), ("temp_filtered", 1),
          ("batt_filtered", 1), ("main_loop_dt", 1), ("cmd_dt", 1), ("motor_cmd", 4), ("motor_forces", 4))
DISCRETE = ("flight_state", "panic_reason", "warnings", "motors_running", "cycle_counter", "last_radio_us")
RUN_DTYPE = np.dtype([("flight_state", "<i4"), ("panic_reason", "<i4"), ("warnings", "<i4"), ("motors_running", "<i4"), ("cycle_counter", "<i4"),
                      ("last_radio_us", "<u8"), ("f", "<f4", (31,))])
DISCRETE_DTYPES = dict(flight_state=np.uint8, panic_reason=np.uint8, warnings=np.uint8, motors_running=np.uint8, cycle_counter=np.uint32,
                       last_radio_us=np.uint64)
assert RUN_DTYPE.itemsize == 152
_TICK = struct.Struct("<iQ iff ifff ifff if i".replace(" ", ""))
_RADIO = struct.Struct("<iQiiiffff")
_PLACE = struct.Struct("<ii4f3fi20fiQ")
PLACE_BITS = dict(est_att4=1, est_ang_vel3=2, imu_initialized=4, lowpass20=8, flight_state=16, last_radio_us=32)
LINE_DTYPE = np.dtype([("clock_us", "<u8"), ("step", "<i4"), ("cycle", "<i4"), ("batt_count", "<i4"), ("gyro_count", "<i4"), ("acc_count", "<i4"),
                       ("temp_count", "<i4"), ("voltage_raw", "<f4"), ("temp_raw", "<f4"), ("voltage_filtered", "<f4")])
VEHICLE_TYPES = (1, 2, 4, 5)
VEHICLE_TICKS = 20


class Recorder:
    """tests/onboard_reference.Vehicle's five methods, writing the call down instead of making it"""

    def __init__(self, t0_us, type_id, vehicle_id, mount=None, volts=None):
        self.ops = [struct.pack("<iQ", CLOCK, int(t0_us)), struct.pack("<iii", INIT, int(type_id), int(vehicle_id) & 0xff)]
        if mount is not None:
            self.ops.append(struct.pack("<ifff", MOUNT, *[float(F(x)) for x in mount]))
        self.volts = volts
        self.kinds = []

    def radio(self, now_us, mtype, flags, floats):
        self.ops.append(_RADIO.pack(CLOCK, int(now_us), RADIO, int(mtype), int(flags), *[float(F(x)) for x in list(floats)[:4]]))

    def set_battery(self, volts):
        self.volts = F(volts)

    def place(self, name, value):
        att, w, imu, lp, state, reset = [0.0] * 4, [0.0] * 3, 0, [0.0] * 20, 0, 0
        if name == "est_att4":
            att = [float(F(x)) for x in value]
        elif name == "est_ang_vel3":
            w = [float(F(x)) for x in value]
        elif name == "imu_initialized":
            imu = int(bool(value))
        elif name == "lowpass20":
            lp = [float(F(x)) for x in value]
        elif name == "flight_state":
            state = int(value)
        elif name == "last_radio_us":
            reset = int(value)
        else:
            raise ValueError(name)
        self.ops.append(_PLACE.pack(PLACE, PLACE_BITS[name], *att, *w, imu, *lp, state, reset))

    def tick(self, T_us, gyro, acc):
        self.ops.append(_TICK.pack(CLOCK, int(T_us), BATTERY, float(self.volts), -1.0, GYRO, *[float(x) for x in gyro], ACC, *[float(x) for x in acc],
                                   TEMP, 25.0, RUN))
        self.kinds.append(RUN)

    def telemetry(self):
        self.ops.append(struct.pack("<i", TELEMETRY))
        self.kinds.append(TELEMETRY)

    def n_ops(self):
        # a packed tick is six calls, a packed radio two
        return sum({_TICK.size: 6, _RADIO.size: 2}.get(len(b), 1) for b in self.ops)


def type_ids(rec):
    """the reference's QuadcopterType of every type record of the flight"""
    return of.TYPE_IDS if len(rec["llist"]) == len(of.TYPE_IDS) else (of.TYPE_IDS[2],)


def call_lists(afa, rec, ticks=None, vehicles=None):
    ids = type_ids(rec)

    def make(i, t0, period, logic, cfg, mount, ty):
        tilted = tuple(float(x) for x in logic["mount"])
        plain = afa.rates_logic_params_from_type(ids[ty])
        placed = tilted != (float(plain.imu_yaw), float(plain.imu_pitch), float(plain.imu_roll))
        volts = F(np.float64(1.2) * np.float64(cfg["threshold"]))         # Quadcopter_T.cpp:72, as tests/onboard_reference.Vehicle
        return Recorder(t0, ids[ty], i, tilted if placed else None, volts)

    fleet, _ = of.drive_scalar(afa, rec, make, ticks, vehicles)
    return fleet


def request(fleet, period=of.PERIOD):
    parts = [struct.pack("<iii", MAGIC, 0, len(fleet))]
    for r in fleet.values():
        parts.append(struct.pack("<fi", float(F(period)), r.n_ops()))
        parts.extend(r.ops)
    return b"".join(parts)


def run_probe(probe, data):
    """one child process on the CPU; a trap (or any other death) of the reference's code fails here by name"""
    out = subprocess.run([probe], input=data, capture_output=True)
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "eigen_trap" not in err, "oracle/_ref/onboard_probe ended with status %r: %s" % (out.returncode, err[-400:])
    return out.stdout


def parse(answer, fleet):
    """-> (fields per tick, {vehicle: [packets of its telemetry reads, uint8 [2, 30]]})"""
    magic, mode, n = struct.unpack_from("<iii", answer, 0)
    assert magic == MAGIC and mode == 0 and n == len(fleet)
    buf = np.frombuffer(answer, np.uint8)
    at, runs, packets = 12, {}, {}
    for i, r in fleet.items():
        kinds = np.array(r.kinds)
        sizes = np.where(kinds == RUN, RUN_DTYPE.itemsize, 60)
        offs = at + np.concatenate([[0], np.cumsum(sizes)[:-1]])
        run_at, tel_at = offs[kinds == RUN], offs[kinds == TELEMETRY]
        runs[i] = buf[run_at[:, None] + np.arange(RUN_DTYPE.itemsize)].copy().view(RUN_DTYPE)[:, 0]
        packets[i] = [buf[o:o + 60].reshape(2, 30).copy() for o in tel_at]
        at += int(sizes.sum())
    assert at == len(answer), (at, len(answer))
    who = list(fleet)
    n_ticks = len(next(iter(runs.values())))
    allruns = np.stack([runs[i] for i in who], axis=1)                   # [ticks, vehicles]
    fields = []
    for k in range(n_ticks):
        row, f, c = {}, allruns[k]["f"], 0
        for name in DISCRETE:
            row[name] = allruns[k][name].astype(DISCRETE_DTYPES[name])
        for name, comps in FLOATS:
            row[name] = f[:, c].copy() if comps == 1 else f[:, c:c + comps].T.copy()
            c += comps
        fields.append(row)
    return fields, packets


def fly_reference(afa, rec, probe=PROBE, ticks=None, vehicles=None):
    """ALL vehicles by default; with `vehicles` the arrays' last axis runs over that list"""
    fleet = call_lists(afa, rec, ticks, vehicles)
    req = request(fleet)
    fields, packets = parse(run_probe(probe, req), fleet)
    telemetry, nth = {}, {i: 0 for i in fleet}
    for k in sorted(rec["events"]):
        if ticks is not None and k > ticks:
            break
        for event in rec["events"][k]:
            if event[0] == "telemetry":
                got = []
                for i in range(event[1], event[1] + event[2]):
                    if i in fleet:
                        got.append(packets[i][nth[i]])
                        nth[i] += 1
                telemetry[(k, event[1], event[2])] = np.stack(got) if got else np.zeros((0, 2, 30), np.uint8)
    return fields, telemetry, hashlib.sha256(req).hexdigest()


# ---- the vehicle mode --------------------------------------------------------------------------------------------------------------
def vehicle_lines(afa, probe=PROBE, types=VEHICLE_TYPES, dt_us=of.DT_US, n_ticks=VEHICLE_TICKS, period=of.PERIOD):
    """Quadcopter_T<Onboard::QuadcopterLogic> of every type, noise off, stepped until the logic has run n_ticks times (and a few
    steps more) -> {type: LINE_DTYPE [n_ticks]}.  The constructor's physical arguments are the package's type record; nothing
    the lines hold depends on them."""
    steps = int(n_ticks * (period * 1e6 / dt_us + 1)) + 8
    b = struct.pack("<iii", MAGIC, 1, len(types))
    for t in types:
        p = afa.params_from_type(t)
        inertia = np.array(list(p.inertia), np.float64).reshape(3, 3)
        b += struct.pack("<iii", t, dt_us, steps)
        b += struct.pack("<33d", float(p.mass), *inertia.reshape(9), *np.linalg.inv(inertia).reshape(9), float(p.arm_length), *list(p.com_error),
                         float(p.motor_min_speed), float(p.motor_max_speed), float(p.prop_thrust_from_speed_sqr), float(p.prop_torque_from_speed_sqr),
                         float(p.motor_time_const), float(p.motor_inertia), *list(p.lin_drag_coeff_b), float(period))
    out = run_probe(probe, b)
    magic, mode, n = struct.unpack_from("<iii", out, 0)
    assert magic == MAGIC and mode == 1 and n == len(types)
    at, lines = 12, {}
    for t in types:
        (count,) = struct.unpack_from("<i", out, at)
        at += 4
        lines[t] = np.frombuffer(out, LINE_DTYPE, count, at)[:n_ticks].copy()
        at += count * LINE_DTYPE.itemsize
        assert len(lines[t]) == n_ticks
    assert at == len(out)
    return lines


def restated_vehicle_lines(afa, types=VEHICLE_TYPES, dt_us=of.DT_US, n_ticks=VEHICLE_TICKS, period=of.PERIOD):
    """the same lines from the restated feed: tests/onboard_reference.TickGate decides the tick, Vehicle.tick hands over battery,
    samples and temperature in Quadcopter_T's order (the samples themselves are not part of a line: zeros)"""
    from tests import gps_imu_reference as gref
    from tests import onboard_reference as orf
    lines = {}
    for t in types:
        logic = oc.logic_record(afa.rates_logic_params_from_type(t))
        cfg = oc.config_from(afa.onboard_default_config(t))
        veh = orf.Vehicle(0, period, logic, cfg, gref.mount_matrix(*logic["mount"]), oc.glibc_math)
        gate = orf.TickGate(veh.clock, period)
        rows, step = [], 0
        while len(rows) < n_ticks:
            step += 1
            veh.clock.now_us += dt_us
            if not gate.fires():
                continue
            veh.tick(veh.clock.now_us, [F(0)] * 3, [F(0), F(0), F(9.81)])
            L = veh.logic
            rows.append((veh.clock.now_us, step, L._cycleCounter, L._count["batt"], L._count["gyro"], L._count["acc"], L._count["temp"], L._voltageRaw,
                         L._tempRaw, L._voltageFiltered))
        lines[t] = np.array(rows, LINE_DTYPE)
    return lines
