"""tests/estimator_flight.py's loop with the FIELD stack's estimator between the vehicle and the offboard side (test
infrastructure): the same orchard, the same start, the same planner settings, and per offboard period

    [step to the logic tick -> imu] x 5 -> measure -> [every 3rd tick: render_engine (the TRUE pose) -> follower.plan] -> follower.tick

(ExampleVehicleStateMachine.cpp:68-77 Predict on every IMU message at 500 Hz, :79-85 UpdateWithMeasurement at 100 Hz,
:816-817 EstGetState = GetCurrentEstimate, no prediction ahead and nothing announced).  Planner inputs, adoption and
tracking fly on the estimate; nothing of the state or of the IMU sample is downloaded in the loop.  What the hooks and the
log hold is downloaded for them alone."""
import numpy as np


def fly_gps(afa, n=48, ticks=100, seed=0, n_candidates=192, rows=6, cols=10, altitude=1.2, plan_every=3, start_planning=0.5,
            on_create=None, on_imu=None, on_measure=None, before_tick=None, after_tick=None, stream=None, image=(320, 240)):
    """on_create(engine, follower, estimator, goal) once; on_imu(now_us, engine, estimator) behind every imu call,
    on_measure(now_us, engine, estimator) behind every measure call; before_tick(tick, now_us, engine, follower, estimator)
    between the plan and the tick, after_tick(...) behind the tick."""
    sc = afa.scenarios
    tris = sc.orchard_mesh(rows=rows, cols=cols, seed=seed)
    scene = afa.Scene(tris)
    cam = afa.camera_default(*image)
    mount = afa.camera_default_mount()
    params = afa.params_from_type(5)
    rng = np.random.default_rng(seed)
    lane = rng.integers(0, rows - 1, n)                      # (the draws of fly_orchard, in its order)
    on_row = rng.random(n) < 0.5
    y0 = np.where(on_row, lane * 4.0 + rng.uniform(-0.3, 0.3, n), lane * 4.0 + 2.0 + rng.uniform(-0.8, 0.8, n))
    pos0 = np.stack([np.full(n, -4.0) + rng.uniform(-1, 0, n), y0, np.full(n, altitude)])
    goal = np.stack([np.full(n, (cols - 1) * 3.0 + 8.0), y0, np.full(n, altitude)])
    att0 = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    e = afa.Ensemble(n, precision=afa.AFE_F32)
    e.set_type_table([params])
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_DECORRELATED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    if stream is not None:
        e.set_stream(stream)
    e.set_state(pos0, np.zeros((3, n)), att0, np.zeros((3, n)), np.full((4, n), sc.hover_speed(params)))
    e.set_rates_commands(np.full(n, 9.81, np.float32), np.zeros((3, n), np.float32))
    buf = afa.DeviceBuffer(n * image[0] * image[1] * 2)
    cfg = afa.planner_default_config(image[0], image[1], cam.depth_scale, cam.focal_length, 2 * params.arm_length,
                                     3 * params.arm_length, 0.5)
    cfg.cost_type = 1
    samples = afa.planner_samples(0, image[0], image[1], n_candidates)
    fol = afa.Follower(e, quadcopter_type=5)                                 # hold = where the vehicles stand
    fol.set_goal(goal)
    est = afa.GpsEstimator(e)                                                # before the first logic tick
    fol.attach_gps_estimator(est)
    if on_create is not None:
        on_create(e, fol, est, goal)

    dt_us = 1000
    log = {"found": []}
    for tick in range(1, ticks + 1):
        for _ in range(5):
            e.step(dt_us, e.steps_until_tick(dt_us))
            est.imu()
            if on_imu is not None:
                on_imu(e.time_us, e, est)
        est.measure()
        now = e.time_us
        if on_measure is not None:
            on_measure(now, e, est)
        if now * 1e-6 >= start_planning and tick % plan_every == 0:
            scene.render_engine(e, cam, mount, out=buf)
            n_found, _, _, _ = fol.plan(cfg, buf, samples)
            log["found"].append(n_found / n)
        if before_tick is not None:
            before_tick(tick, now, e, fol, est)
        fol.tick()
        if after_tick is not None:
            after_tick(tick, now, e, fol, est)
    st = e.get_state()
    log["planned"] = fol.get_plans()["planned"].astype(bool)
    log["last_sent"] = fol.get_command()[1]
    log["estimator"], log["estimator_info"] = est.state(), est.info()
    log["pos"], log["vel"], log["att"], log["time_us"] = st["pos"], st["vel"], st["att"], e.time_us
    fol.close()
    est.close()
    buf.close()
    if stream is not None:
        e.set_stream(None)
    e.close()
    log["found"] = np.array(log["found"])
    log["pos0"], log["goal"] = pos0, goal
    return log
