"""Flights of the onboard flight computer whose truth is known (test infrastructure): 16 CF_MINIQUAD vehicles hovering at 5 m, IMU
noise on (0.1 rad/s, 0.2 m/s^2) under the counter policy so that the CPU oracle and the engine draw the same samples, 0.6 s.

  mode "rates"   swinging rates commands (2 rad/s about x and y at 1.5 Hz, a phase per vehicle), a new one every 10 ticks: the
                 vehicles tilt by up to 0.41 rad; how far is the ESTIMATED tilt from the TRUE tilt?
  mode "acc"     the hover command of the acceleration mode (0, 0, 0) with a yaw rate of 0.5 rad/s: the onboard attitude loop holds
                 the vehicle level while it turns and drifts on at the velocity it starts with (a few m/s, as the ensembles of
                 tests/test_gpu_logic.py move: the parity definition is relative, with floors made for vehicles that move)

The rotors start at the float value of the hover speed, the very number the first command holds, on both sides.

  fly_oracle(ora, afa, mode)        the CPU oracle's rigid body and IMU with tests/onboard_checker.py as the vehicle's firmware
  fly_engine(afa, precision, mode)  the engine with the device onboard computer: [step to the tick -> onboard.tick]

Both return `trace`: (raw gyro, raw acc, motor commands) behind every tick, the final true state, `tilt_err`: the worst
|estimated tilt - true tilt| [rad] over all ticks and vehicles (the tilt is the angle between the body's z axis and the vertical;
yaw is unobservable without UWB), and `tilt_max`: the largest true tilt."""
import numpy as np

from tests import onboard_checker as oc

N, DT_US, SEED, TICKS = 16, 1000, 21, 300
PERIOD = 1.0 / 500.0
HEIGHT = 5.0
F = np.float32


def command(mode, k, n):
    """the message sent before tick k (k = 1, 11, 21, ...) -> (type, floats [4, n]) or None"""
    if (k - 1) % 10:
        return None
    if mode == "acc":
        return oc.MSG_ACCELERATION, np.vstack([np.zeros((3, n)), np.full((1, n), 0.5)]).astype(F)
    t = (k - 1) * 0.002
    ph = 2 * np.pi * np.arange(n) / n
    w = np.stack([2.0 * np.sin(2 * np.pi * 1.5 * t + ph), 2.0 * np.cos(2 * np.pi * 1.5 * t + ph), np.zeros(n)])
    return oc.MSG_RATES, np.vstack([np.full((1, n), 9.81), w]).astype(F)


def start(afa, mode):
    """-> (hover speed as the float command holds it, initial velocity [3, N])"""
    hover = float(F(afa.params_from_type(5).hover_speed))
    vel = np.random.default_rng(SEED).normal(0, 2.0, (3, N)) if mode == "acc" else np.zeros((3, N))
    return hover, vel


def _packets(afa, mtype, floats):
    if mtype == oc.MSG_ACCELERATION:
        return np.stack([afa.radio_create_acceleration_command(0, floats[0:3, i], floats[3, i]) for i in range(floats.shape[1])])
    return np.stack([afa.radio_create_rates_command(0, floats[0, i], floats[1:4, i]) for i in range(floats.shape[1])])


def _sent(afa, mtype, floats):
    """what the radio codec leaves of the floats"""
    pk = _packets(afa, mtype, floats)
    return pk, np.array([list(afa.radio_decode(p).floats)[:4] for p in pk], F).T


def fly_oracle(ora, afa, mode, math=oc.glibc_math, ticks=TICKS):
    p = ora.params_from_type(5)
    b = ora.Batch(N, [p])
    b.pos[2] = HEIGHT
    hover, b.vel[:] = start(afa, mode)
    b.motor_speed[:] = hover
    b.motor_cmd[:] = F(hover)
    ck = oc.Onboard(N, PERIOD, np.zeros(N, int), [oc.logic_record(afa.rates_logic_params_from_type(5))],
                    [oc.config_from(afa.onboard_default_config(5))], t0_us=0, math=math)
    steps = ticks * 2 + 20
    gate = afa.plan_ticks(PERIOD, 0, DT_US, steps)[0]          # the engine's step numbering: its step j is the reference's Run() j + 1
    # (ora.clock_ticks also lists Run() 0, whose dt is 0 and which integrates nothing: one physics step too many for a comparison of positions)
    k, err, tilt_max, trace = 1, 0.0, 0.0, []
    for s in range(steps):
        if gate[s]:
            msg = command(mode, k, N)
            if msg is not None:
                ck.deliver(s * DT_US, np.arange(N), msg[0], 0, _sent(afa, *msg)[1])
        ora.step_counter(b, DT_US, 1, [gate[s]], tick_base=k - 1, seed=SEED, first_global=0)
        if not gate[s]:
            continue
        ck.tick(s * DT_US, b.gyro, b.acc)
        b.motor_cmd[:] = ck.motor_cmd
        trace.append((b.gyro.copy(), b.acc.copy(), ck.motor_cmd.copy()))
        true = oc.tilt_from_vertical(b.att)
        err = max(err, float(np.abs(oc.tilt_from_vertical(ck.att) - true).max()))
        tilt_max = max(tilt_max, float(true.max()))
        k += 1
        if k > ticks:
            break
    return dict(pos=b.pos.copy(), vel=b.vel.copy(), att=b.att.copy(), ang_vel=b.ang_vel.copy(), tilt_err=err, tilt_max=tilt_max,
                states=ck.state.copy(), trace=trace)


def fly_engine(afa, precision, mode, step_mode=None, ticks=TICKS):
    params = afa.params_from_type(5)
    e = afa.Ensemble(N, precision=precision)
    e.set_type_table([params])
    e.set_logic_period(PERIOD)
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_COUNTER)
    e.set_noise_seed(SEED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    if step_mode is not None:
        e.set_step_mode(step_mode)
    pos = np.zeros((3, N))
    pos[2] = HEIGHT
    att = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, N))
    hover, vel = start(afa, mode)
    e.set_state(pos, vel, att, np.zeros((3, N)), np.full((4, N), hover))
    e.set_motor_cmds(np.full((4, N), hover, np.float32))
    ob = afa.Onboard(e, quadcopter_type=5)
    err, tilt_max, trace = 0.0, 0.0, []
    try:
        for k in range(1, ticks + 1):
            n_steps = e.steps_until_tick(DT_US)
            if n_steps > 1:
                e.step(DT_US, n_steps - 1)
            msg = command(mode, k, N)                        # (before the ticking step, as the oracle's loop sends it)
            if msg is not None:
                ob.radio(_packets(afa, *msg))
            e.step(DT_US, 1)
            ob.tick()
            trace.append(e.get_imu() + (e.get_motor_cmds(),))
            true = oc.tilt_from_vertical(e.get_state()["att"])
            err = max(err, float(np.abs(oc.tilt_from_vertical(ob.get(fields=["est_att"])["est_att"]) - true).max()))
            tilt_max = max(tilt_max, float(true.max()))
        st = e.get_state()
        states = ob.get(fields=["flight_state"])["flight_state"]
    finally:
        ob.close()
        e.close()
    return dict(pos=st["pos"], vel=st["vel"], att=st["att"], ang_vel=st["ang_vel"], tilt_err=err, tilt_max=tilt_max, states=states,
                trace=trace)
