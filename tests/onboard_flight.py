"""The onboard flight computer flown on the engine beside its numpy checker (test infrastructure).  The loop is the vehicle's:

    [step to the logic tick -> onboard.tick]      optionally beside a follower or a stage machine that keeps sending

  make_engine(afa, n, precision, mode)   mixed type records, the third with a tilted IMU mount; hovering under a rates command
  script(afa, n, w0)                     the scripted flight of the CPU and GPU tests: tick -> events applied BEFORE the steps to it
  fly_device(afa, ...)                   the script on the device; records the engine's raw IMU sample and clock of every tick
                                         (what teacher-forces the checker), every field, command, counter and telemetry byte
  fly_beside(afa, e, ob, ticks, ...)     the loop beside a live sender: a stage machine's or a follower's tick every few ticks
  replay(afa, record, math)              the same script through tests/onboard_checker.py on the recorded samples
  replay_scalar(afa, record, math)       ... and through tests/onboard_reference.py, one vehicle at a time
  drive_scalar(afa, record, make)        the driver under replay_scalar, for any object with the scalar Vehicle's five methods
  synthetic_record(afa)                  a record without a device, for the CPU tests

Events of the script:
  ("rates", first, thrust [k], w [3, k])     afe_set_rates_commands
  ("radio", first, packets [k, 23])          afe_onboard_radio
  ("engine_radio", first, packets)           afe_set_commands_from_radio
  ("battery", first, volts [k])              afe_onboard_set_battery
  ("onboard_state", first, fields)           afe_onboard_set_state
  ("late_rates", first, thrust, w)           afe_set_rates_commands BETWEEN the ticking step and the onboard tick
  ("telemetry", first, count)                afe_onboard_telemetry, read AFTER the tick
Ticks SLOW_FROM .. SLOW_TO are reached in ONE step of 3 ms each (a tick every 3 ms: the main-loop monitor notices; the gate's
backlog then fires a tick every step for a while)."""
import numpy as np

from tests import onboard_checker as oc

N = 130                      # two full waves and two lanes
TYPE_IDS = (5, 1, 4)
TILTED = (0.3, -0.2, 0.25)   # the third record's IMU mount (yaw, pitch, roll)
DT_US = 1000
PERIOD = 1.0 / 500.0
SILENCE_FROM = 30            # the tick after which the silent range hears nothing any more
SLOW_FROM, SLOW_TO = 300, 320
OVERRIDE_AT = 765            # (T is past 1.5 s there: a radio timer set back to 0 has run out)
EDGE_AT = 752                # the last silent vehicle's radio timer stands at EXACTLY 1 500 000 us at this tick: no time-out yet (placed at 750)
NAN_FIRST = 37               # synthetic_record alone: this plain vehicle's FIRST accelerometer sample is NaN (acosf of a NaN cosine)
TICKS = 1200                 # 2.4 s: the radio time-out (1.5 s after the last message at tick SILENCE_FROM) falls at two thirds


def tick_clocks(ticks=TICKS):
    """(now, T, after) of every tick under the loop of fly_device -- step until the vehicle's tick gate fires (Quadcopter_T.cpp:159-160,
    tests/onboard_reference.TickGate: more than a period since the gate's timer, which then moves on by ONE period); T is the clock
    at the start of the ticking step.  1 ms steps under the 2 ms period: the first tick fires on the third step, then on every
    second; 3 ms steps fire one each and leave the gate 1 ms further behind every time, so that after the slow stretch every 1 ms
    step fires a tick until the backlog is gone"""
    from tests import onboard_reference as orf
    clock = orf.Clock(0)
    gate = orf.TickGate(clock, PERIOD)
    out = []
    for k in range(1, ticks + 1):
        dt = 3 * DT_US if SLOW_FROM <= k < SLOW_TO else DT_US
        now = clock.now_us
        while True:
            clock.now_us += dt
            if gate.fires():
                break
        out.append((now, clock.now_us - dt, clock.now_us))
    return out


def records(afa, single=False):
    plist = [afa.params_from_type(t) for t in TYPE_IDS]
    llist = [afa.rates_logic_params_from_type(t) for t in TYPE_IDS]
    for rec in (plist[2], llist[2]):
        rec.imu_yaw, rec.imu_pitch, rec.imu_roll = TILTED
    clist = [afa.onboard_default_config(t) for t in TYPE_IDS]
    if single:
        return [plist[2]], [llist[2]], [clist[2]]
    return plist, llist, clist


def groups(n):
    """who does what in the script (index arrays; for n == 1 the one vehicle flies rates and nothing else)"""
    k = np.arange(n)
    if n < 64:
        e = np.zeros(0, int)
        return dict(turn=e, turn_suppressed=e, silent=e, flat=e, kill=e, idle=e, acc_hover=e, acc_general=e, acc_cut=e, both_flat=e, both_turned=e, chatty=e,
                    long=e, late=e)
    return dict(turn=k[3:6], turn_suppressed=k[6:7], silent=k[60:66], flat=k[70:74], kill=k[80:83], idle=k[83:85], acc_hover=k[90:93],
                acc_general=k[93:97], acc_cut=k[97:99], both_turned=k[110:111], both_flat=k[111:113], chatty=k[100:102], long=k[115:116], late=k[120:122])


def make_engine(afa, n, precision, mode=None, noise=True, seed=3):
    """hovering at 40 m under a rates command; the `turn` vehicles spin about x at 9 rad/s and are commanded to go on"""
    single = mode == afa.AFE_STEP_RESIDENT or n == 1
    plist, llist, clist = records(afa, single)
    types = np.zeros(n, np.uint8) if single else ((np.arange(n) + 2) % 3).astype(np.uint8)
    e = afa.Ensemble(n, precision=precision)
    e.set_type_table(plist)
    e.set_vehicle_types(types)
    e.set_logic_period(PERIOD)
    e.set_imu_noise(noise, 0.1, 0.2, afa.AFE_SEED_COUNTER)
    e.set_noise_seed(seed)
    e.set_rates_logic(llist)
    if mode is not None:
        e.set_step_mode(mode)
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-5, 5, (3, n)) + np.array([[30.0], [-20.0], [40.0]])
    att = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    w = np.zeros((3, n))
    g = groups(n)
    spin = np.concatenate([g["turn"], g["turn_suppressed"]])
    w[0, spin] = 9.0
    hover = np.array([p.hover_speed for p in plist])[types]
    e.set_state(pos, np.zeros((3, n)), att, w, np.tile(hover, (4, 1)))
    e.set_motor_cmds(np.tile(hover, (4, 1)).astype(np.float32))
    return e, types, llist, clist, w.astype(np.float32)


def script(afa, n, w0):
    """tick k -> events applied after onboard tick k - 1 and before the steps to tick k"""
    g = groups(n)
    ev = {}
    add = lambda k, *e: ev.setdefault(k, []).append(e)            # noqa: E731
    everyone = np.arange(n)
    thrust = np.full(n, 9.81, np.float32)
    listeners = np.setdiff1d(everyone, np.concatenate([g["silent"], g["kill"], g["idle"], g["acc_hover"], g["acc_general"], g["acc_cut"],
                                                       g["turn_suppressed"]]))
    # the sender: a rates command every 10 ticks (20 ms), in maximal runs of consecutive vehicles
    def runs(idx):
        idx = np.sort(idx)
        cut = np.flatnonzero(np.diff(idx) != 1) + 1
        return [r for r in np.split(idx, cut) if r.size]
    for k in range(2, TICKS + 1, 10):
        who = np.setdiff1d(everyone, g["turn_suppressed"]) if k <= SILENCE_FROM else listeners
        for r in runs(who):
            add(k, "rates", int(r[0]), thrust[r], w0[:, r])
    if n >= 64:
        # the suppressing flag rides on a radio packet (quantised command); sent every 10 ticks like the others, one tick later
        for k in range(3, TICKS + 1, 10):
            i = int(g["turn_suppressed"][0])
            add(k, "radio", i, np.stack([afa.radio_create_rates_command(oc.FLAG_DISABLE_CHECKS, 9.81, w0[:, i])]))
        add(40, "radio", int(g["kill"][0]), np.stack([afa.radio_create_simple_command(oc.MSG_KILL)] * g["kill"].size))
        add(60, "engine_radio", int(g["kill"][0]), np.stack([afa.radio_create_rates_command(0, 9.81, np.zeros(3, np.float32))] * g["kill"].size))   # ignored: KILLED
        # the last of the killed hears the kill with its voltage filter at 1 V: a reason, but KILLED is no safety-critical state
        flat20 = np.zeros((20, 1), np.float32)
        flat20[[2, 5, 8, 11]], flat20[12:16], flat20[16:20] = 9.81, 1.0, 25.0
        add(40, "onboard_state", int(g["kill"][-1]), dict(lowpass20=flat20))
        # a delivery between the ticking step and the onboard tick is stamped later than the tick's clock: it waits for the next tick
        late = g["late"]
        add(500, "late_rates", int(late[0]), thrust[late], w0[:, late])
        add(40, "radio", int(g["idle"][0]), np.stack([afa.radio_create_simple_command(oc.MSG_IDLE)] * g["idle"].size))
        acc = lambda a, yaw, k: np.stack([afa.radio_create_acceleration_command(0, np.array(a, np.float32), yaw)] * k)   # noqa: E731
        for k in range(41, TICKS + 1, 10):
            add(k, "radio", int(g["acc_hover"][0]), acc([0, 0, 0], 0.0, g["acc_hover"].size))
            add(k, "radio", int(g["acc_general"][0]), acc([1.0, -0.5, 0.3], 0.2, g["acc_general"].size))
            add(k, "radio", int(g["acc_cut"][0]), acc([0, 0, -6.0], 0.0, g["acc_cut"].size))
        for k in range(7, TICKS + 1, 10):                          # twice the expected rate: the command-rate monitor notices
            r = g["chatty"]
            add(k, "rates", int(r[0]), thrust[r], w0[:, r])
        add(100, "battery", int(g["flat"][0]), np.full(g["flat"].size, 1.0, np.float32))
        # two reasons at one tick, the later check wins: a radio timer set back to 0 has run out at OVERRIDE_AT, and at the same tick
        # the estimate is upside down (one vehicle) or the voltage filter stands at 1 V (two vehicles)
        add(OVERRIDE_AT, "onboard_state", int(g["both_turned"][0]), dict(est_att4=np.array([[0.0], [1.01], [0.0], [0.0]], np.float32),
                                                                         last_radio_us=np.zeros(1, np.uint64)))
        # (not a unit quaternion: the expected accelerometer direction is 2 % too long, the cosine falls below -1; and above +1:)
        add(OVERRIDE_AT, "onboard_state", int(g["long"][0]), dict(est_att4=np.array([[1.01], [0.0], [0.0], [0.0]], np.float32)))
        k2 = g["both_flat"].size
        lp20 = np.zeros((20, k2), np.float32)
        lp20[[2, 5, 8, 11]] = 9.81
        lp20[12:16] = 1.0
        lp20[16:20] = 25.0
        add(OVERRIDE_AT, "onboard_state", int(g["both_flat"][0]), dict(lowpass20=lp20, last_radio_us=np.zeros(k2, np.uint64)))
        # the time-out is `>`: a radio timer that reads exactly 1 500 000 us at tick EDGE_AT lets that tick pass, the next one panics
        add(EDGE_AT - 2, "onboard_state", int(g["silent"][-1]), dict(last_radio_us=np.array([tick_clocks(EDGE_AT)[-1][1] - 1500000], np.uint64)))
        # PANIC is a sink: a later command to a vehicle that panicked is ignored (the flat ones keep hearing the sender)
        add(200, "telemetry", 63, 3)
        add(400, "telemetry", 0, n)
        add(TICKS, "telemetry", 0, n)
    else:
        add(200, "telemetry", 0, n)
    return ev


def _decode(afa, packets):
    ms = [afa.radio_decode(p) for p in packets]
    return (np.array([m.type for m in ms], np.uint8), np.array([m.flags for m in ms], np.uint8),
            np.array([list(m.floats)[:4] for m in ms], np.float32).T)


def fly_device(afa, precision, mode=None, n=N, ticks=TICKS, noise=True, nan_vehicle=None):
    e, types, llist, clist, w0 = make_engine(afa, n, precision, mode, noise)
    ob = afa.Onboard(e, cfgs=clist)
    ev = script(afa, n, w0)
    rec = dict(n=n, types=types, llist=llist, clist=clist, events=ev, ticks=[], fields=[], cmds=[], counts=[], telemetry={}, t0=e.time_us,
               running=[])
    try:
        if nan_vehicle is not None:
            st = e.get_state()
            st["pos"][:, nan_vehicle] = np.nan
            st["ang_vel"][:, nan_vehicle] = np.nan
            e.set_state(st["pos"], st["vel"], st["att"], st["ang_vel"], st["motor_speed"])
        for k in range(1, ticks + 1):
            post = []
            for event in ev.get(k, []):
                if event[0] == "rates":
                    e.set_rates_commands(event[2], event[3], first=event[1], count=len(event[2]))
                elif event[0] == "radio":
                    ob.radio(event[2], first=event[1])
                elif event[0] == "engine_radio":
                    e.set_commands_from_radio(event[2], first=event[1])
                elif event[0] == "battery":
                    ob.set_battery(event[2], first=event[1])
                elif event[0] == "onboard_state":
                    ob.set_state(first=event[1], **event[2])
                else:
                    post.append(event)
            now = e.time_us
            dt = 3 * DT_US if SLOW_FROM <= k < SLOW_TO else DT_US
            e.step(dt, e.steps_until_tick(dt))
            rec["running"].append(bool(e.persistent_running))
            for event in post:
                if event[0] == "late_rates":
                    e.set_rates_commands(event[2], event[3], first=event[1], count=len(event[2]))
            counts = ob.tick(count=True)
            gyro, acc = e.get_imu()
            rec["ticks"].append((now, e.time_us - dt, e.time_us, gyro, acc))
            rec["fields"].append(ob.get())
            rec["cmds"].append(e.get_motor_cmds())
            rec["counts"].append(counts)
            for event in post:
                if event[0] == "telemetry":
                    rec["telemetry"][(k, event[1], event[2])] = ob.telemetry(event[1], event[2])
    finally:
        ob.close()
        e.close()
    return rec


def fly_beside(afa, e, ob, ticks, sender=None, every=10, before_steps=None, after_tick=None, dt_us=DT_US):
    """The loop beside a live sender.  sender(k): called before the steps to tick k = 1, 1 + every, ... (a stage machine's or a
    follower's tick, with whatever the caller wants to read back from it) -- BEHIND onboard tick k - 1, so that its delivery is
    stamped between two onboard ticks; before_steps(k): anything else to do there; after_tick(k, T): behind onboard tick k, whose
    clock was T."""
    for k in range(1, ticks + 1):
        if sender is not None and (k - 1) % every == 0:
            sender(k)
        if before_steps is not None:
            before_steps(k)
        e.step(dt_us, e.steps_until_tick(dt_us))
        ob.tick()
        if after_tick is not None:
            after_tick(k, e.time_us - dt_us)


def replay(afa, rec, math=oc.glibc_math, ticks=None):
    """the recorded flight through the checker -> (fields, cmds, counts, telemetry, checker)"""
    n = rec["n"]
    ck = oc.Onboard(n, PERIOD, rec["types"], [oc.logic_record(p) for p in rec["llist"]], [oc.config_from(c) for c in rec["clist"]],
                    t0_us=rec["t0"], math=math)
    fields, cmds, counts, telemetry = [], [], [], {}
    for k, (now, T, after, gyro, acc) in enumerate(rec["ticks"][:ticks], start=1):
        post = []
        for event in rec["events"].get(k, []):
            if event[0] == "rates":
                cnt = len(event[2])
                ck.deliver(now, np.arange(event[1], event[1] + cnt), oc.MSG_RATES, 0, np.vstack([event[2][None], event[3]]))
            elif event[0] in ("radio", "engine_radio"):
                mtype, flags, floats = _decode(afa, event[2])
                ck.deliver(now, np.arange(event[1], event[1] + len(mtype)), mtype, flags, floats)
            elif event[0] == "battery":
                ck.set_battery(event[2], event[1])
            elif event[0] == "onboard_state":
                ck.set_state(event[1], **event[2])
            else:
                post.append(event)
        for event in post:
            if event[0] == "late_rates":
                cnt = len(event[2])
                ck.deliver(after, np.arange(event[1], event[1] + cnt), oc.MSG_RATES, 0, np.vstack([event[2][None], event[3]]))
        counts.append(ck.tick(T, gyro, acc))
        fields.append(ck.fields())
        cmds.append(ck.motor_cmd.copy())
        for event in post:
            if event[0] == "telemetry":
                telemetry[(k, event[1], event[2])] = ck.telemetry(event[1], event[2])
    return fields, cmds, counts, telemetry, ck


def first_tick_in_state(fields, vehicle, state):
    for k, f in enumerate(fields, start=1):
        if f["flight_state"][vehicle] == state:
            return k
    return None


def synthetic_record(afa, n=N, ticks=TICKS, seed=5, single=False):
    """a record like fly_device's without a device: the tick clock of 1 ms steps under a 2 ms period (3 ms in the slow stretch) and
    a made-up IMU -- gravity along the sensor's z with noise on every second vehicle (the others measure it exactly: the
    correction axis vanishes), the spin of the turning vehicles on the gyro; vehicle NAN_FIRST measures a NaN acceleration at the
    first tick (the alignment's cosine is a NaN, no errno: its attitude estimate is NaN for good).  Nothing physical: the CPU tests
    compare restatements."""
    single = single or n == 1                              # (single: the fleet of the resident grid, one tilted record for everyone)
    plist, llist, clist = records(afa, single)
    types = np.zeros(n, np.uint8) if single else ((np.arange(n) + 2) % 3).astype(np.uint8)
    g = groups(n)
    w0 = np.zeros((3, n), np.float32)
    w0[0, np.concatenate([g["turn"], g["turn_suppressed"]]).astype(int)] = 9.0
    rng = np.random.default_rng(seed)
    noisy = (np.arange(n) % 2 == 1)
    rec = dict(n=n, types=types, llist=llist, clist=clist, events=script(afa, n, w0), ticks=[], t0=0)
    for k, (now, T, after) in enumerate(tick_clocks(ticks), start=1):
        gyro = (w0 + np.where(noisy, rng.normal(0, 0.1, (3, n)), 0.0)).astype(np.float32)
        acc = (np.array([[0.0], [0.0], [9.81]]) + np.where(noisy, rng.normal(0, 0.2, (3, n)), 0.0)).astype(np.float32)
        if k == 1 and n > NAN_FIRST:
            acc[:, NAN_FIRST] = np.nan
        rec["ticks"].append((now, T, after, gyro, acc))
    return rec


def drive_scalar(afa, rec, make_vehicle, ticks=None, vehicles=None, after_tick=None):
    """THE driver of one-vehicle-at-a-time objects through the recorded flight: make_vehicle(i, t0, period, logic, cfg, mount,
    type_index) -> an object with tests/onboard_reference.Vehicle's radio / set_battery / place / tick / telemetry.  With Vehicle
    itself this is replay_scalar; with a recorder it is the call list the reference's own class is given
    (tests/onboard_probe.py).  after_tick(k, fleet) is called behind the ticks of tick k.  -> (fleet, telemetry): telemetry[(k,
    first, count)] = [what telemetry() returned, per vehicle of the range that is in the fleet]"""
    from tests import gps_imu_reference as gref
    F = np.float32
    n = rec["n"]
    who = list(range(n)) if vehicles is None else list(vehicles)
    logic = [oc.logic_record(p) for p in rec["llist"]]
    cfgs = [oc.config_from(c) for c in rec["clist"]]
    mounts = [gref.mount_matrix(*r["mount"]) for r in logic]
    fleet = {i: make_vehicle(i, rec["t0"], PERIOD, logic[int(rec["types"][i])], cfgs[int(rec["types"][i])], mounts[int(rec["types"][i])],
                             int(rec["types"][i])) for i in who}

    def deliver(event, when):
        if event[0] in ("rates", "late_rates"):
            for j in range(len(event[2])):
                if event[1] + j in fleet:
                    fleet[event[1] + j].radio(when, oc.MSG_RATES, 0, [event[2][j]] + list(event[3][:, j]))
        else:
            mtype, flags, floats = _decode(afa, event[2])
            for j in range(len(mtype)):
                if event[1] + j in fleet:
                    fleet[event[1] + j].radio(when, mtype[j], flags[j], floats[:, j])

    telemetry = {}
    for k, (now, T, after, gyro, acc) in enumerate(rec["ticks"][:ticks], start=1):
        late = []
        for event in rec["events"].get(k, []):
            if event[0] in ("rates", "radio", "engine_radio"):
                deliver(event, now)
            elif event[0] == "late_rates":
                late.append(event)
            elif event[0] == "battery":
                for j, v in enumerate(event[2]):
                    if event[1] + j in fleet:
                        fleet[event[1] + j].set_battery(F(v))
            elif event[0] == "onboard_state":
                for j in range(np.asarray(next(iter(event[2].values()))).shape[-1]):
                    if event[1] + j not in fleet:
                        continue
                    for name, a in event[2].items():
                        fleet[event[1] + j].place(name, np.asarray(a)[..., j])
        for i, veh in fleet.items():
            veh.tick(T, gyro[:, i], acc[:, i])
        if after_tick is not None:
            after_tick(k, fleet)
        for event in late:
            deliver(event, after)
        for event in rec["events"].get(k, []):
            if event[0] == "telemetry":                          # GetTelemetryDataPackets clears the warnings of the range
                telemetry[(k, event[1], event[2])] = {event[1] + j: fleet[event[1] + j].telemetry() for j in range(event[2]) if event[1] + j in fleet}
    return fleet, telemetry


def replay_scalar(afa, rec, math=oc.glibc_math, ticks=None, vehicles=None, with_telemetry=False):
    """the recorded flight through tests/onboard_reference.py, one vehicle at a time -> per tick dicts like Onboard.fields() plus
    "motor_cmd", for `vehicles` (default: all); with_telemetry: -> (rows, {(k, first, count): {vehicle: (packet 1, packet 2)}})"""
    from tests import onboard_reference as orf
    F = np.float32
    out = []

    def after_tick(k, fleet):
        row = {}
        for i, veh in fleet.items():
            L = veh.logic
            row[i] = dict(flight_state=L._state, panic_reason=L._firstPanicReason, warnings=L._telWarnings, est_att=np.array(L._kf._att, F),
                          est_ang_vel=np.array(L._kf._angVel, F), acc_filtered=np.array(L._acc.GetValue(), F),
                          gyro_filtered=np.array(L._gyro.GetValue(), F), temp_filtered=F(L._temp.GetValue()), batt_filtered=F(L._voltageFiltered),
                          main_loop_dt=F(L._monitorMainLoopPeriod.lpDt), cmd_dt=F(L._monitorCmdRate.lpDt),
                          motor_forces=np.array(L._desMotorForcesForTelemetry, F), cycle_counter=L._cycleCounter,
                          last_radio_us=L._timeSinceLastRadioMessage.last, motors_running=int(L.GetAreMotorsRunning()),
                          motor_cmd=np.array(L._desMotorSpeeds, F))
        out.append(row)

    _, telemetry = drive_scalar(afa, rec, lambda i, t0, period, logic, cfg, mount, ty: orf.Vehicle(t0, period, logic, cfg, mount, math),
                                ticks, vehicles, after_tick)
    return (out, telemetry) if with_telemetry else out
