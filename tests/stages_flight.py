"""A whole mission of the flight stage machine whose truth is known (test infrastructure): 24 CF_MINIQUAD vehicles at rest
at ground level wait, spool up, take off to 1 m, fly the circle of trajectory 3 for 1.2 s, land and idle, with the GPS +
IMU estimator between the vehicle and the machine, IMU noise on (0.1 rad/s, 0.2 m/s^2) under the counter policy so that
the CPU oracle and the engine draw the same samples.  The loop is the field node's:

    [step to the logic tick -> gps.imu] x 10, gps.measure after every fifth -> stages.tick          (500 / 100 / 50 Hz)

  fly_oracle(ora, afa)    the CPU oracle's closed loop (oracle_py.ClosedLoopBatch: the reference's rigid body, IMU and rates
                          logic) with the numpy checkers of the estimator and of the stage machine
  fly_engine(afa, prec)   the engine with the device estimator and the device stage machine

Neither the engine nor the oracle has a ground.  "At rest on the ground" is z = 0 at rest with the motors at hover speed and a
hover command in force, which stands in for the ground until the machine's first delivery (WaitForStart's message changes
nothing); from SpoolUp's quarter of a g on the vehicle sags until the take-off catches it, and after the idle command of
Complete it falls, so the final height is taken at the tick a vehicle turns Complete.

The stage times are shortened through the config so that the oracle's flight stays within a few seconds: spool-up 0.1 s,
take-off 0.6 s, get-into-action 0.4 s, landing speed 1 m/s; the start signal comes at tick 10 (0.2 s, twenty GPS updates for
the estimator to settle) and the stop signal 1.2 s into Flight.

Both return stages [ticks, n] (after every tick), `off_track`: the largest distance [m] of the true position from the
commanded point over the last second of Flight, and `final_height`: the largest |z| [m] at the tick a vehicle turns Complete."""
import numpy as np

from tests import gps_estimator_checker as gc
from tests import stages_checker as sc

N, DT_US, SEED = 24, 1000, 13
PERIOD = 1.0 / 500.0
TICKS, START_TICK, FLIGHT_S = 215, 10, 1.2
SHORT = dict(spool_up_time=0.1, takeoff_time=0.6, get_into_action_time=0.4, landing_speed=1.0)


def layout(n=N):
    """start positions (a grid on the ground, 1.5 m apart), desired positions 1 m above them, circle centres on them"""
    k = np.arange(n)
    pos = np.stack([(k % 6) * 1.5 - 3.75, (k // 6) * 1.5 - 2.25, np.zeros(n)])
    des = pos + np.array([[0.0], [0.0], [1.0]])
    att = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    return pos, att, des, pos[0:2].copy()


def mission_config(traj_id=3):
    cfg = sc.default_config(traj_id)
    cfg.update(SHORT)
    return cfg


class _Judge:
    """what both flights record, from the machine's fields and the true position behind every tick"""

    def __init__(self, n):
        self.stages, self.flight_from, self.off, self.final = [], np.full(n, -1), [], np.full(n, np.nan)

    def tick(self, k, stage, last_pos, true_pos):
        prev = self.stages[-1] if self.stages else np.zeros_like(stage)
        self.stages.append(stage.copy())
        entered = (stage == sc.FLIGHT) & (prev != sc.FLIGHT)
        self.flight_from[entered] = k
        flying = (prev == sc.FLIGHT)                         # this tick ran Flight: last_pos is its commanded point
        late = flying & (k - self.flight_from > int(round((FLIGHT_S - 1.0) / 0.02)))
        if late.any():
            self.off.append(float(np.sqrt(((true_pos - last_pos) ** 2).sum(0))[late].max()))
        done = (stage == sc.COMPLETE) & (prev != sc.COMPLETE)
        self.final[done] = true_pos[2, done]

    def result(self):
        return dict(stages=np.stack(self.stages), off_track=max(self.off) if self.off else np.nan,
                    final_height=float(np.nanmax(np.abs(self.final))) if np.isfinite(self.final).any() else np.nan,
                    flight_from=self.flight_from.copy())


def _stop_now(judge, k):
    """the stop signal: FLIGHT_S after the first vehicle entered Flight (they all enter at the same tick)"""
    first = judge.flight_from[judge.flight_from >= 0]
    return first.size > 0 and k - first.min() >= int(round(FLIGHT_S / 0.02))


def fly_oracle(ora, afa, math=sc.glibc_math, traj_id=3):
    p = ora.params_from_type(5)
    b = ora.Batch(N, [p])
    pos0, att0, des, centre = layout()
    b.pos[:], b.att[:] = pos0, att0
    hover = np.sqrt(p.mass * 9.81 / (4 * p.k_thrust))
    b.motor_speed[:] = hover
    b.motor_cmd[:] = np.float32(hover)
    cl = ora.ClosedLoopBatch(b, [ora.logic_params_from_type(5, PERIOD)], PERIOD, counter=dict(seed=SEED, first_global=0))
    lp = afa.rates_logic_params_from_type(5)
    sampler = gc.Sampler(N, PERIOD, [(lp.imu_yaw, lp.imu_pitch, lp.imu_roll)], np.zeros(N, int), [lp.gyro_lowpass_cutoff])
    est = gc.Estimator(N, gc.default_config(), lambda op, x: math(op, x) if op < 2 else math(5, x.astype(np.float32)).astype(np.float64))
    cfg = mission_config(traj_id)
    st = sc.new_state(N, cfg)
    st["desired_pos"], st["centre"] = des, centre
    line = sc.DelayLine(cfg["delay_us"])
    cl.set_rates_cmd(np.full(N, 9.81, np.float32), np.zeros((3, N), np.float32))
    judge = _Judge(N)
    steps = TICKS * 20 + 20                                  # (the logic's float period is a hair over 2 ms: a tick now and then comes a step late)
    _, ticks = ora.clock_ticks(DT_US * 1e-6, PERIOD, steps)
    n_ticks = k = 0
    for s in range(steps):
        cl.step(DT_US * 1e-6, [ticks[s]])
        if not ticks[s]:
            continue
        now = (s + 1) * DT_US
        n_ticks += 1
        est.imu(now, *sampler.sample(b.gyro, b.acc))
        if n_ticks % 5 == 0:
            est.measure(now, b.pos)
        if n_ticks % 10 == 0:
            k += 1
            state = est.state()
            since = (np.uint64(now) - state["last_update_us"].astype(np.uint64)).astype(np.float64) * 1e-6
            e13 = state["est"]
            msg = sc.tick(st, cfg, now, e13[0:3], e13[3:6], e13[6:10], since, k >= START_TICK, _stop_now(judge, k), math)
            due = line.tick(now, msg)
            if due is not None:
                types, sent = due
                for i, ls in enumerate(cl.states):
                    if types[i] == sc.MSG_RATES:
                        cl.L.ora_logic_set_rates_cmd(ls, float(sent[0, i]), (np.ctypeslib.ctypes.c_float * 3)(*[float(x) for x in sent[1:4, i]]))
                    elif types[i] in (sc.MSG_IDLE, sc.MSG_KILL):
                        ls.have_rates_cmd = 0
            judge.tick(k, st["stage"], st["last_pos"], b.pos)
            if k == TICKS:
                break
    return judge.result()


def fly_engine(afa, precision, traj_id=3, mode=None, box=None, push=None):
    """box: (min_corner, max_corner) in place of the default's; push: (vehicle, force3 [N], from_tick): an external force on
    one vehicle from that tick on.  -> the judge's result, and `have` [ticks, n]: the engine's have bytes behind every tick"""
    params = afa.params_from_type(5)
    e = afa.Ensemble(N, precision=precision)
    e.set_type_table([params])
    e.set_logic_period(PERIOD)
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_COUNTER)
    e.set_noise_seed(SEED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    if mode is not None:
        e.set_step_mode(mode)
    pos0, att0, des, centre = layout()
    hover = params.hover_speed
    e.set_state(pos0, np.zeros((3, N)), att0, np.zeros((3, N)), np.full((4, N), hover))
    e.set_motor_cmds(np.full((4, N), hover, np.float32))
    e.set_rates_commands(np.full(N, 9.81, np.float32), np.zeros((3, N), np.float32))
    est = afa.GpsEstimator(e)
    cdict = mission_config(traj_id)
    if box is not None:
        cdict["min_corner"], cdict["max_corner"] = np.asarray(box[0], float), np.asarray(box[1], float)
    s = afa.FlightStages(e, cfg=sc.config_into(cdict, afa.stages_default_config(5)))
    s.attach_gps_estimator(est)
    s.set_desired_position(des)
    s.set_centre(centre)
    judge, have, safety = _Judge(N), [], []
    try:
        n_ticks = k = 0
        while k < TICKS:
            e.step(DT_US, e.steps_until_tick(DT_US))
            est.imu()
            n_ticks += 1
            if n_ticks % 5 == 0:
                est.measure()
            if n_ticks % 10 == 0:
                k += 1
                if push is not None and k == push[2]:
                    f = np.zeros((3, N))
                    f[:, push[0]] = push[1]
                    e.set_external_force(f)
                s.tick(k >= START_TICK, _stop_now(judge, k))
                got = s.get(fields=["stage", "last_pos", "safety"])
                judge.tick(k, got["stage"], got["last_pos"], e.get_state()["pos"])
                have.append(e.get_rates_commands()[2])
                safety.append(got["safety"])
    finally:
        s.close()
        est.close()
        e.close()
    out = judge.result()
    out["have"], out["safety"] = np.stack(have), np.stack(safety)
    return out
