"""tests/follower_flight.py's loop with the reference's estimator between the vehicle and the offboard side (test
infrastructure): the same orchard, the same start, the same planner settings, and per offboard period

    step x 5 -> measure -> step x 5 -> measure -> predict(0.03)
             -> [every 3rd tick: render_engine (the TRUE pose, as AirSim gets it) -> follower.plan] -> follower.tick

(Simulator/Rappids_Simulator/main.cpp:451-457 the mocap system at 200 Hz, :468-469 GetPrediction, :647-649
SetPredictedValues -- the attached tick's announce).  Planner inputs, adoption and tracking fly on the estimator's
prediction; nothing of the state is downloaded in the loop.  What the log holds is downloaded for the log alone."""
import numpy as np

from tests.orchard_flight import clearance


def fly_estimated(afa, n=48, seconds=3.0, seed=0, n_candidates=192, rows=6, cols=10, altitude=1.2, plan_every=3, log_every=2,
                  start_planning=0.5, on_create=None, on_measure=None, before_tick=None, after_tick=None, stream=None):
    """on_create(engine, follower, estimator, goal) once; on_measure(now_us, engine, estimator) behind every measure call;
    before_tick(tick, now_us, engine, follower, estimator) between the plan and the tick, after_tick(...) behind the tick."""
    sc = afa.scenarios
    tris, layout = sc.orchard_mesh(rows=rows, cols=cols, seed=seed, return_layout=True)
    scene = afa.Scene(tris)
    cam = afa.camera_default(320, 240)
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
    buf = afa.DeviceBuffer(n * 240 * 320 * 2)
    cfg = afa.planner_default_config(320, 240, cam.depth_scale, cam.focal_length, 2 * params.arm_length,
                                     3 * params.arm_length, 0.5)            # main.cpp:167-169
    cfg.cost_type = 1
    samples = afa.planner_samples(0, 320, 240, n_candidates)                 # the reference re-seeds with 0 per plan
    fol = afa.Follower(e, quadcopter_type=5)                                 # hold = where the vehicles stand
    fol.set_goal(goal)
    est = afa.Estimator(e)
    fol.attach_estimator(est)
    if on_create is not None:
        on_create(e, fol, est, goal)

    dt_us, period_off = 1000, 0.01
    log = {"t": [], "pos": [], "vel": [], "pred": [], "trunk": [], "canopy": [], "found": []}
    n_ticks = int(round(seconds / period_off))
    for tick in range(1, n_ticks + 1):
        for half in (1, 2):
            e.step(dt_us, 5)
            est.measure()
            if on_measure is not None:
                on_measure((tick - 1) * 10 * dt_us + half * 5 * dt_us, e, est)
        est.predict(0.03)
        now = tick * 10 * dt_us
        t = now * 1e-6
        if t >= start_planning and tick % plan_every == 0:
            scene.render_engine(e, cam, mount, out=buf)
            n_found, _, _, _ = fol.plan(cfg, buf, samples)
            log["found"].append(n_found / n)
        if before_tick is not None:
            before_tick(tick, now, e, fol, est)
        fol.tick()
        if after_tick is not None:
            after_tick(tick, now, e, fol, est)
        if log_every and tick % log_every == 0:
            st = e.get_state()
            trunk, canopy = clearance(layout, st["pos"])
            log["t"].append(t)
            log["pos"].append(st["pos"].copy())
            log["vel"].append(st["vel"].copy())
            log["pred"].append(est.prediction())
            log["trunk"].append(trunk)
            log["canopy"].append(canopy)
    planned = fol.get_plans()["planned"].astype(bool)
    sent = fol.get_command()[1]
    final = est.state()
    info = est.info()
    fol.close()
    est.close()
    buf.close()
    if stream is not None:
        e.set_stream(None)
    e.close()
    for k in ("t", "pos", "vel", "pred", "trunk", "canopy", "found"):
        log[k] = np.array(log[k])
    log["pos0"], log["goal"], log["layout"], log["planned"], log["last_sent"] = pos0, goal, layout, planned, sent
    log["estimator"], log["estimator_info"] = final, info
    return log
