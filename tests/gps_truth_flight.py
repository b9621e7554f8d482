"""A flight whose truth is known, for judging the GPS + IMU estimate against something that is NOT its own restatement
(test infrastructure).  24 CF_MINIQUAD vehicles start level and at rest at hover and fly 0.6 s under rates commands that
change every offboard period (10 ms): body rates of up to 1 rad/s swinging at 1.5 to 3 Hz, thrust within 5 % of hover.
IMU noise is on (0.1 rad/s, 0.2 m/s^2) under the counter policy, so the CPU oracle and the engine draw the same samples.
The estimator is fed as the field node feeds it: Predict on every logic tick, UpdateWithMeasurement with the true position
after every fifth.

  fly_oracle(ora, math)   the CPU oracle's closed loop (oracle_py.ClosedLoopBatch: the reference's rigid body, IMU and
                          rates logic) with the numpy checker
  fly_engine(afa, prec)   the engine with the device estimator

Both return the largest position [m], velocity [m/s] and tilt [rad] error of the estimate against the true state, taken
behind every update from the first on."""
import numpy as np

from tests import gps_estimator_checker as gc

N, STEPS, DT_US, SEED = 24, 600, 1000, 11
PERIOD = 1.0 / 500.0


def start(n=N):
    rng = np.random.default_rng(SEED)
    pos = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(3, 8, n)])
    att = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    return pos, att


def commands(k, n=N):
    """the rates command in force during offboard period k: (thrust_norm [n], des_ang_vel [3, n]) float32"""
    rng = np.random.default_rng(SEED + 1)
    amp = rng.uniform(0.2, 1.0, (3, n)) * np.array([[1.0], [1.0], [0.3]])
    freq = rng.uniform(1.5, 3.0, (3, n))
    phase = rng.uniform(0, 2 * np.pi, (3, n))
    t = k * 0.01
    w = amp * np.sin(2 * np.pi * freq * t + phase)
    thrust = 9.81 * (1 + 0.05 * np.sin(2 * np.pi * 1.0 * t + phase[0]))
    return thrust.astype(np.float32), w.astype(np.float32)


def _z_axis(q):
    z = np.stack([2 * q[1] * q[3] + 2 * q[0] * q[2], 2 * q[2] * q[3] - 2 * q[0] * q[1], q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3]])
    return z / np.sqrt((z * z).sum(0))


def errors(est13, pos, vel, att):
    """largest |position|, |velocity| and tilt error over the vehicles"""
    ep = np.sqrt(((est13[0:3] - pos) ** 2).sum(0)).max()
    ev = np.sqrt(((est13[3:6] - vel) ** 2).sum(0)).max()
    tilt = np.arccos(np.clip((_z_axis(est13[6:10]) * _z_axis(att)).sum(0), -1.0, 1.0)).max()
    return float(ep), float(ev), float(tilt)


def _worse(worst, now):
    return tuple(max(a, b) for a, b in zip(worst, now))


def fly_oracle(ora, afa, math=gc.glibc_math):
    p = ora.params_from_type(5)
    b = ora.Batch(N, [p])
    b.pos[:], b.att[:] = start()
    hover = np.sqrt(p.mass * 9.81 / (4 * p.k_thrust))
    b.motor_speed[:] = hover
    b.motor_cmd[:] = np.float32(hover)
    cl = ora.ClosedLoopBatch(b, [ora.logic_params_from_type(5, PERIOD)], PERIOD, counter=dict(seed=SEED, first_global=0))
    lp = afa.rates_logic_params_from_type(5)
    sampler = gc.Sampler(N, PERIOD, [(lp.imu_yaw, lp.imu_pitch, lp.imu_roll)], np.zeros(N, int), [lp.gyro_lowpass_cutoff])
    chk = gc.Estimator(N, gc.default_config(), math)
    _, ticks = ora.clock_ticks(DT_US * 1e-6, PERIOD, STEPS)
    worst, n_ticks, n_updates = (0.0, 0.0, 0.0), 0, 0
    cl.set_rates_cmd(*commands(0))
    for s in range(STEPS):
        cl.step(DT_US * 1e-6, [ticks[s]])
        if not ticks[s]:
            continue
        now = (s + 1) * DT_US
        n_ticks += 1
        chk.imu(now, *sampler.sample(b.gyro, b.acc))
        if n_ticks % 5 == 0:
            chk.measure(now, b.pos)
            n_updates += 1
            worst = _worse(worst, errors(chk.state()["est"], b.pos, b.vel, b.att))
            cl.set_rates_cmd(*commands(n_ticks // 5))
    return dict(worst=worst, n_ticks=n_ticks, n_updates=n_updates, counts=chk.count)


def fly_engine(afa, precision, mode=None):
    params = afa.params_from_type(5)
    e = afa.Ensemble(N, precision=precision)
    e.set_type_table([params])
    e.set_logic_period(PERIOD)
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_COUNTER)
    e.set_noise_seed(SEED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    if mode is not None:
        e.set_step_mode(mode)
    pos, att = start()
    hover = params.hover_speed
    e.set_state(pos, np.zeros((3, N)), att, np.zeros((3, N)), np.full((4, N), hover))
    e.set_motor_cmds(np.full((4, N), hover, np.float32))
    e.set_rates_commands(*commands(0))
    est = afa.GpsEstimator(e)
    worst, n_ticks, n_updates = (0.0, 0.0, 0.0), 0, 0
    try:
        while True:
            k = e.steps_until_tick(DT_US)
            if e.time_us + k * DT_US > STEPS * DT_US:
                break
            e.step(DT_US, k)
            est.imu()
            n_ticks += 1
            if n_ticks % 5 == 0:
                est.measure()
                n_updates += 1
                st = e.get_state()
                worst = _worse(worst, errors(est.state()["est"], st["pos"], st["vel"], st["att"]))
                e.set_rates_commands(*commands(n_ticks // 5))
    finally:
        est.close()
        e.close()
    return dict(worst=worst, n_ticks=n_ticks, n_updates=n_updates)
