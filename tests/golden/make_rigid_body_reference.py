"""tests/golden/rigid_body_reference.npz: what the REFERENCE's own Quadcopter_T::Run computed (oracle/_ref/rigid_body_probe:
Quadcopter_T.cpp and Motor.cpp compiled where they lie against the storage-only oracle/eigen_store, instantiated with a
logic stub that records the IMU floats and replays a command script) on 96 vehicles in five (dt, logic period) groups --
every case's full state, rotor speeds, last IMU sample, held commands and tick count after steps 1, 2, 10 and the last, and
the group's tick pattern.  The fixture holds the cases' inputs too, so the tests read nothing else.

    python tests/golden/make_rigid_body_reference.py     # needs oracle/_ref/rigid_body_probe (built where the reference is)

The one Eigen operation of the path, inertiaMatrix.inverse() (Quadcopter_T.cpp:20), is INJECTED: the probe hands back the
nine numbers of the request, which are ora_params_init's.  Inertia class A (power-of-two diagonal, exact under any sane
algorithm) is therefore pinned without condition, classes B (the shipped types' diagonals) and C (full SPD tensors) given
the inverse, which tests/test_rigid_body_reference.py bounds against the exact one.

A second fixture, tests/golden/rigid_body_closed_loop.npz, records the same probe with the loop CLOSED: Quadcopter_T
instantiated with a logic that composes the reference's own onboard headers (LowPassFilterSecondOrder, QuadcopterAngular-
VelocityController, QuadcopterMixer, QuadcopterConstants) in QuadcopterLogic.cpp's order -- 12 vehicles of the four shipped
types, 150 steps, rates commands that arrive after 7 steps and change twice and reach the mixer's total-thrust cap and both
per-propeller clamps.  The glue between those headers is the probe's own reading and stays unpinned.

Also the loader and the helpers the two test files share (tests/test_rigid_body_reference.py on the CPU,
tests/test_gpu_rigid_body_reference.py on the device); the tests never run the probe except to check staleness."""
import importlib
import io
import os
import struct
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(HERE, "rigid_body_reference.npz")
PROBE = os.path.join(ROOT, "oracle", "_ref", "rigid_body_probe")

MAGIC = 0x31425152
MIN_ANGLE = 4.84813681e-6        # Rotation.hpp:39, FromRotationVector's small-angle branch
SANE_TURN = 0.5                  # rad per step, tests/campaigns/step_campaign.py's own sanity bound
Z_CLEAR = 1e-4                   # fp32 cases: every recorded pos.z is exactly 0 or above this
# (dt_us, logic period) from tests/campaigns/step_campaign.py's DTS_US / PERIODS, and dt 0 = Quadcopter_T.cpp:88-90's return
GROUPS = [dict(dt_us=1000, period=1 / 500, steps=60, n=68),
          dict(dt_us=2000, period=1 / 500, steps=40, n=8),
          dict(dt_us=250, period=1 / 1000, steps=120, n=8),
          dict(dt_us=1000, period=0.0033, steps=50, n=8),
          dict(dt_us=0, period=1 / 500, steps=12, n=4)]
N_SETS = 4                       # command rows per case: before the first tick, then three script rows
KINDS = ("flight", "fall_through", "rest_thrust", "touch_start", "no_contact", "slow_below", "slow_above")
SPECIAL = ("fall_through", "rest_thrust", "touch_start", "no_contact", "slow_below", "slow_above")
PARAM_FIELDS = ("mass", "inertia", "inverse", "arm", "com", "min_speed", "max_speed", "k_thrust", "k_torque", "tau", "J", "drag")


def checkpoints(steps):
    return [1, 2, 10, steps]


def script_rows(n_ticks):
    """which command set ScriptLogic::Run number r leaves: set 1, from a third of the ticks set 2, from two thirds set 3"""
    c1, c2 = max(1, n_ticks // 3), max(2, 2 * n_ticks // 3)
    return np.array([1 if r < c1 else 2 if r < c2 else 3 for r in range(max(n_ticks, 1))], np.int32)


def _pow2(x):
    return float(2.0 ** np.round(np.log2(x)))


def make_cases():
    """the 96 cases: dicts of plain floats.  Deterministic (PCG64), one generator per case."""
    afa = importlib.import_module("agri-fly_amd")
    from oracle import oracle_py as ora
    cases = []
    for gi, g in enumerate(GROUPS):
        dt = g["dt_us"] * 1e-6
        for k in range(g["n"]):
            rng = np.random.Generator(np.random.PCG64(20261019 * 100 + gi * 1000 + k))
            kind = "flight"
            if gi == 0 and k < 12:
                kind = SPECIAL[k % 6]
            elif gi in (1, 2, 3) and k == 0:
                kind = "fall_through"
            type_id = [5, 1, 2, 4][k % 4]
            p = afa.params_from_type(type_id)
            inertia = np.array(p.inertia).reshape(3, 3)
            icls = "ABC"[(k + gi) % 3]
            motor = ("reference", "reference", "lag", "lag_J")[(k // 3 + gi) % 4]
            if kind in ("slow_below", "slow_above"):
                icls, motor = "A", "reference"
            if icls == "A":
                inertia = np.diag([_pow2(inertia[0, 0]), _pow2(inertia[1, 1]), _pow2(inertia[2, 2])])
            elif icls == "C":         # a full symmetric positive-definite tensor, as in tests/campaigns/step_campaign.py
                a = rng.normal(size=(3, 3)) * 0.15
                inertia = inertia + a @ a.T * inertia[0, 0]
                inertia = 0.5 * (inertia + inertia.T)
            tau = float(rng.uniform(0.008, 0.06)) if motor != "reference" else 0.0
            J = float(rng.uniform(1e-8, 2e-6)) * (inertia[0, 0] / 16e-6) if motor == "lag_J" else 0.0
            plain = kind in ("slow_below", "slow_above")
            com = [0.0] * 3 if plain or k % 2 == 0 else [float(x) for x in rng.normal(0, 1.5e-3, 3)]
            drag = [0.0] * 3 if plain or k % 3 == 0 else [float(x) for x in rng.uniform(0.02, 0.3, 3)]
            min_speed = float(p.motor_min_speed) if k % 2 else float(rng.uniform(50, 200))
            max_speed = float(p.motor_max_speed)
            mass = float(p.mass) * (1.0 if k % 4 == 0 else float(rng.uniform(0.8, 1.25)))
            kf, ktau = float(p.prop_thrust_from_speed_sqr), float(p.prop_torque_from_speed_sqr)
            o = ora.params_init(mass, inertia.reshape(9), float(p.arm_length), com, min_speed, max_speed, kf, ktau, tau, J, drag)
            hover = float(np.sqrt(mass * 9.81 / (4.0 * kf)))

            att = rng.normal(size=4)
            att /= np.linalg.norm(att)
            pos = [float(rng.normal(0, 2)), float(rng.normal(0, 2)), float(rng.uniform(5, 9))]
            vel = [float(x) for x in rng.normal(0, 1.0, 3)]
            w = [float(x) for x in rng.normal(0, 2.0, 3)]
            force = [float(x) for x in rng.normal(0, 0.3 * mass * 9.81, 3)] if k % 2 else [0.0] * 3
            torque = [float(x) for x in rng.normal(0, 0.02 * mass * 9.81 * p.arm_length, 3)] if k % 3 == 1 else [0.0] * 3
            cmds = hover * (1.0 + rng.uniform(-0.2, 0.2, (N_SETS, 4)))
            # below the minimum, above the maximum and negative, on single rotors of single command sets
            if k % 5 == 1:
                cmds[1, 0] = 0.25 * min_speed if min_speed > 0 else 0.0
            if k % 5 == 2:
                cmds[2, 1] = 1.05 * max_speed
            if k % 5 == 3:
                cmds[rng.integers(0, N_SETS), 2] = -50.0
            if k % 5 == 4:
                cmds[0, 3] = 1.02 * max_speed
            if kind != "flight":
                att = np.array([1.0, 0.0, 0.0, 0.0]) if plain else att * [1, 0.05, 0.05, 1]    # nearly upright
                att = att / np.linalg.norm(att)
                force, torque = [0.0] * 3, [0.0] * 3
            if kind == "fall_through":        # starts above the ground at a third of the hover thrust, meets it within 15 ms
                pos[2], vel[2] = 0.012, -1.0
                cmds = hover * np.sqrt(1 / 3.0) * np.ones((N_SETS, 4))
            elif kind == "rest_thrust":       # on the ground, thrust upward and below the weight: contact at every step
                pos[2], vel[2], w = 0.0, 0.0, [0.0] * 3
                cmds = hover * np.sqrt(rng.uniform(0.3, 0.8, (N_SETS, 1))) * np.ones((1, 4))
            elif kind == "touch_start":       # z exactly 0 with v_z < 0 at the start
                pos[2], vel[2] = 0.0, -0.5
                cmds = hover * 0.5 * np.ones((N_SETS, 4))
            elif kind == "no_contact":        # z <= 0 with v_z >= 0: Quadcopter_T.cpp:146's second operand is false
                pos[2], vel[2] = 0.0, 1.5
                cmds = hover * np.ones((N_SETS, 4)) * (1.0 + rng.uniform(0, 0.1, (N_SETS, 1)))
            elif plain:                        # a turn about z that no torque changes: every step on one side of MIN_ANGLE
                w = [0.0, 0.0, (0.5 if kind == "slow_below" else 2.0) * MIN_ANGLE / max(dt, 1e-3)]
                cmds = hover * np.ones((N_SETS, 4)) * (1.0 + rng.uniform(-0.1, 0.1, (N_SETS, 1)))
            cases.append(dict(group=gi, kind=KINDS.index(kind), inertia_class="ABC".index(icls), type_id=type_id,
                              mass=mass, inertia=inertia.reshape(9).copy(), inverse=np.array(o.inertia_inv), arm=float(p.arm_length),
                              com=np.array(com), min_speed=min_speed, max_speed=max_speed, k_thrust=kf, k_torque=ktau, tau=tau, J=J,
                              drag=np.array(drag), pos=np.array(pos), vel=np.array(vel), att=np.array(att), ang_vel=np.array(w),
                              ext_force=np.array(force), ext_torque=np.array(torque), cmd_sets=cmds.astype(np.float32)))
    return cases


# ---- the probe's request and answer -----------------------------------------------------------------------------------
def encode_request(cases, n_rows_of_group):
    b = struct.pack("<2i", MAGIC, len(cases))
    for c in cases:
        g = GROUPS[c["group"]]
        cp = checkpoints(g["steps"])
        rows = c["cmd_sets"][script_rows(n_rows_of_group[c["group"]])]
        b += struct.pack("<5i", c["type_id"], g["dt_us"], g["steps"], len(cp), len(rows))
        b += struct.pack("<33d", c["mass"], *c["inertia"], *c["inverse"], c["arm"], *c["com"], c["min_speed"], c["max_speed"],
                         c["k_thrust"], c["k_torque"], c["tau"], c["J"], *c["drag"], g["period"])
        b += struct.pack("<19d", *c["pos"], *c["vel"], *c["att"], *c["ang_vel"], *c["ext_force"], *c["ext_torque"])
        b += np.asarray(c["cmd_sets"][0], "<f4").tobytes() + np.asarray(cp, "<i4").tobytes() + np.ascontiguousarray(rows, "<f4").tobytes()
    return b


REC = np.dtype([("step", "<i4"), ("ticks", "<i4"), ("pos", "<f8", 3), ("vel", "<f8", 3), ("att", "<f8", 4), ("ang_vel", "<f8", 3),
                ("motor_speed", "<f8", 4), ("gyro", "<f4", 3), ("acc", "<f4", 3), ("cmd", "<f4", 4)])


def decode_answer(b, cases):
    magic, n = struct.unpack_from("<2i", b, 0)
    assert magic == MAGIC and n == len(cases)
    off, out = 8, []
    for c in cases:
        g = GROUPS[c["group"]]
        tick = np.frombuffer(b, np.uint8, g["steps"], off).copy()
        off += g["steps"]
        rec = np.frombuffer(b, REC, len(checkpoints(g["steps"])), off).copy()
        off += rec.nbytes
        out.append((tick, rec))
    assert off == len(b)
    return out


def run_probe(probe, request):
    """the probe twice on the same request: the bytes must be identical"""
    outs = []
    for _ in range(2):
        r = subprocess.run([probe], input=request, stdout=subprocess.PIPE)
        assert r.returncode == 0, r.returncode
        outs.append(r.stdout)
    assert outs[0] == outs[1], "the probe gave different bytes on the same request"
    return outs[0]


def make_rigid_body_reference(probe=PROBE, verbose=False):
    cases = make_cases()
    # pass 1 finds each group's number of ticks (the script's rows are laid out over them), pass 2 records
    first = decode_answer(run_probe(probe, encode_request(cases, [1] * len(GROUPS))), cases)
    n_ticks = [0] * len(GROUPS)
    for c, (tick, _) in zip(cases, first):
        n_ticks[c["group"]] = int(tick.sum())
    ans = decode_answer(run_probe(probe, encode_request(cases, [max(t, 1) for t in n_ticks])), cases)
    ticks = []
    for gi, g in enumerate(GROUPS):
        mine = [a[0] for c, a in zip(cases, ans) if c["group"] == gi]
        assert all(np.array_equal(t, mine[0]) for t in mine) and int(mine[0].sum()) == n_ticks[gi]
        ticks.append(mine[0])
    rec = np.stack([a[1] for a in ans])                  # [case, checkpoint]
    fx = dict(group_dt_us=np.array([g["dt_us"] for g in GROUPS], np.int32), group_period=np.array([g["period"] for g in GROUPS], np.float64),
              group_steps=np.array([g["steps"] for g in GROUPS], np.int32), group_ticks=np.array(n_ticks, np.int32),
              tick_offset=np.concatenate([[0], np.cumsum([len(t) for t in ticks])]).astype(np.int32), tick=np.concatenate(ticks),
              sigma_gyro=np.float64(0.1), sigma_acc=np.float64(0.2))
    for k in ("group", "kind", "inertia_class", "type_id"):
        fx[k] = np.array([c[k] for c in cases], np.int32)
    for k in PARAM_FIELDS + ("pos", "vel", "att", "ang_vel", "ext_force", "ext_torque"):
        fx["in_" + k] = np.array([c[k] for c in cases], np.float64)
    fx["cmd_sets"] = np.stack([c["cmd_sets"] for c in cases])
    for k in REC.names:
        fx["ref_" + k] = np.ascontiguousarray(rec[k])
    fx["fp32_ok"] = fp32_ok(fx)
    check_coverage(fx)
    if verbose:
        for gi, g in enumerate(GROUPS):
            m = fx["group"] == gi
            print("group %d: dt %4d us, period %.4f, %3d steps, %2d ticks, %2d cases, worst |w| dt %.3g rad" % (
                gi, g["dt_us"], g["period"], g["steps"], n_ticks[gi], m.sum(),
                np.linalg.norm(fx["ref_ang_vel"][m], axis=2).max() * g["dt_us"] * 1e-6))
    return fx


def fp32_ok(fx):
    """cases an fp32 engine is compared on: every recorded pos.z exactly 0 or above Z_CLEAR (so float arithmetic cannot
    legitimately take the other side of the contact branch, Quadcopter_T.cpp:146)"""
    z = fx["ref_pos"][:, :, 2]
    return np.all((z == 0.0) | (z > Z_CLEAR), axis=1)


def check_coverage(fx):
    """what the fixture must hold before it is committed: every line of Run() is reached, and the caps on the inputs"""
    n = len(fx["group"])
    assert 64 <= n <= 100
    assert np.bincount(fx["group"]).max() > 64                        # a ragged second wave on the device
    dt = fx["group_dt_us"][fx["group"]] * 1e-6
    moving = dt > 0
    turn = np.linalg.norm(fx["ref_ang_vel"], axis=2) * dt[:, None]
    assert turn.max() <= SANE_TURN, turn.max()                        # no case is excluded from any comparison
    assert np.isfinite(fx["ref_pos"]).all() and np.isfinite(fx["ref_att"]).all()
    ref_model = (fx["in_tau"] == 0) & (fx["in_J"] == 0)
    assert ref_model.sum() >= 20 and ((fx["in_tau"] > 0) & (fx["in_J"] == 0)).sum() >= 10 and (fx["in_J"] > 0).sum() >= 10
    cs, lo, hi = fx["cmd_sets"], fx["in_min_speed"][:, None, None], fx["in_max_speed"][:, None, None]
    assert ((cs < lo) & (cs >= 0)).any(axis=(1, 2)).sum() >= 5 and (cs > hi).any(axis=(1, 2)).sum() >= 10 and (cs < 0).any(axis=(1, 2)).sum() >= 5
    assert np.any(fx["in_ext_force"] != 0, axis=1).sum() >= 20 and np.any(fx["in_ext_torque"] != 0, axis=1).sum() >= 10
    d = fx["in_drag"]
    assert ((d[:, 0] != d[:, 1]) & (d[:, 1] != d[:, 2]) & (d[:, 0] != d[:, 2])).sum() >= 20 and np.any(fx["in_com"] != 0, axis=1).sum() >= 20
    assert all((fx["inertia_class"] == c).sum() >= 15 for c in range(3))
    I = fx["in_inertia"].reshape(n, 3, 3)
    a_cls = fx["inertia_class"] == 0
    assert np.all(np.frexp(I[a_cls][:, [0, 1, 2], [0, 1, 2]])[0] == 0.5) and np.all(I[a_cls] * (1 - np.eye(3)) == 0)
    assert np.all(I[fx["inertia_class"] == 1] * (1 - np.eye(3)) == 0) and np.all(np.abs(I[fx["inertia_class"] == 2] * (1 - np.eye(3))).sum(axis=(1, 2)) > 0)
    # both sides of FromRotationVector's small-angle branch: the turn of the first step, and whole rollouts on one side
    turn0 = np.linalg.norm(fx["in_ang_vel"], axis=1) * dt
    below, above = fx["kind"] == KINDS.index("slow_below"), fx["kind"] == KINDS.index("slow_above")
    assert below.sum() >= 2 and above.sum() >= 2
    assert np.all(turn0[below] < MIN_ANGLE) and np.all(turn[below] < MIN_ANGLE) and np.all(fx["ref_att"][below] == fx["in_att"][below][:, None, :])
    assert np.all(turn0[above] >= MIN_ANGLE) and np.all(turn0[above] < 4 * MIN_ANGLE) and np.any(fx["ref_att"][above][:, -1] != fx["in_att"][above], axis=1).all()
    # ground contact
    z, vz = fx["ref_pos"][:, :, 2], fx["ref_vel"][:, :, 2]
    kind = lambda name: fx["kind"] == KINDS.index(name)
    assert kind("fall_through").sum() >= 4 and np.all(z[kind("fall_through")][:, 0] > Z_CLEAR) and np.all(z[kind("fall_through")][:, -1] == 0)
    assert np.all(z[kind("rest_thrust")] == 0) and np.all(vz[kind("rest_thrust")] == 0) and np.all(fx["ref_motor_speed"][kind("rest_thrust")] > 0)
    assert np.all(fx["in_pos"][kind("touch_start"), 2] == 0) and np.all(fx["in_vel"][kind("touch_start"), 2] < 0) and np.all(z[kind("touch_start")] == 0)
    assert np.all(fx["in_pos"][kind("no_contact"), 2] <= 0) and np.all(fx["in_vel"][kind("no_contact"), 2] >= 0) and np.all(z[kind("no_contact")] > Z_CLEAR)
    for name in SPECIAL:
        assert kind(name).sum() >= 2, name
    # commands change at ticks; the dt 0 group never moves and never ticks
    moved = fx["ref_cmd"][:, 0] != fx["ref_cmd"][:, -1]
    assert moved.any(axis=1)[moving].sum() >= 60
    still = ~moving
    assert still.sum() >= 4 and np.all(fx["ref_ticks"][still] == 0) and np.all(fx["ref_pos"][still] == fx["in_pos"][still][:, None, :])
    assert np.all(fx["ref_motor_speed"][still] == 0) and np.all(fx["group_ticks"][fx["group_dt_us"] == 0] == 0)
    assert np.all(fx["group_ticks"][fx["group_dt_us"] > 0] >= 10)
    # every case is compared in fp32 but the ones that start in exact touch and lift off (none does) -- i.e. every case
    assert np.all(fx["fp32_ok"] | kind("touch_start"))


def write_fixture(fx, path=FIXTURE):
    """an .npz whose bytes depend on its arrays alone (np.savez stamps the time of day into the archive)"""
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(fx):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(fx[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


# ---- the closed loop --------------------------------------------------------------------------------------------------
CL_FIXTURE = os.path.join(HERE, "rigid_body_closed_loop.npz")
MAGIC_CHAIN = 0x31435152
CL = dict(dt_us=1000, period=1 / 500, steps=150, n=12, cmd_steps=(8, 61, 111))     # a command is handed over BEFORE that step
CL_CHECKPOINTS = [1, 2, 8, 10, 30, 60, 61, 62, 70, 110, 111, 112, 120, 150]
CL_REC = np.dtype(REC.descr + [("force", "<f4", 4)])


def make_closed_loop_cases():
    afa = importlib.import_module("agri-fly_amd")
    from oracle import oracle_py as ora
    cases = []
    for j in range(CL["n"]):
        rng = np.random.Generator(np.random.PCG64(20261019 * 100 + 9000 + j))
        type_id, variant = [5, 1, 2, 4][j % 4], j // 4
        p = afa.params_from_type(type_id)
        lp = ora.logic_params_from_type(type_id, CL["period"])
        o = ora.params_init(p.mass, list(p.inertia), p.arm_length, list(p.com_error), p.motor_min_speed, p.motor_max_speed,
                            p.prop_thrust_from_speed_sqr, p.prop_torque_from_speed_sqr, p.motor_time_const, p.motor_inertia,
                            list(p.lin_drag_coeff_b))
        att = rng.normal(size=4) * [1, 0.1, 0.1, 0.3] + [3, 0, 0, 0]
        att /= np.linalg.norm(att)
        cap = float(lp.max_cmd_total_thrust) / float(lp.mass)          # thrust_norm at the mixer's total-thrust cap
        thrust = [9.81 + rng.normal(0, 0.5), 9.81 + rng.normal(0, 1.0), 9.81 + rng.normal(0, 0.5)]
        w = rng.normal(0, 0.5, (3, 3))
        if variant == 1:            # beyond the total-thrust cap, then back
            thrust[1] = 1.3 * cap
        if variant == 2:            # rate steps that drive single propellers into both clamps
            w[0] = rng.choice([-1, 1], 3) * [25.0, 20.0, 8.0]
            w[2] = -w[0]
            thrust[0] = 0.75 * cap
        rows = np.array([[CL["cmd_steps"][k], thrust[k], *w[k]] for k in range(3)], np.float32)
        cases.append(dict(type_id=type_id, mass=float(p.mass), inertia=np.array(p.inertia), inverse=np.array(o.inertia_inv), arm=float(p.arm_length),
                          com=np.array(p.com_error), min_speed=float(p.motor_min_speed), max_speed=float(p.motor_max_speed),
                          k_thrust=float(p.prop_thrust_from_speed_sqr), k_torque=float(p.prop_torque_from_speed_sqr),
                          tau=float(p.motor_time_const), J=float(p.motor_inertia), drag=np.array(p.lin_drag_coeff_b),
                          pos=np.array([rng.normal(0, 2), rng.normal(0, 2), rng.uniform(20, 25)]), vel=rng.normal(0, 0.5, 3), att=att,
                          ang_vel=rng.normal(0, 0.6, 3), ext_force=rng.normal(0, 0.05 * p.mass * 9.81, 3), ext_torque=np.zeros(3), rows=rows))
    return cases


def make_closed_loop_reference(probe=PROBE):
    from oracle import oracle_py as ora
    cases = make_closed_loop_cases()
    b = struct.pack("<2i", MAGIC_CHAIN, len(cases))
    for c in cases:
        b += struct.pack("<5i", c["type_id"], CL["dt_us"], CL["steps"], len(CL_CHECKPOINTS), len(c["rows"]))
        b += struct.pack("<33d", c["mass"], *c["inertia"], *c["inverse"], c["arm"], *c["com"], c["min_speed"], c["max_speed"],
                         c["k_thrust"], c["k_torque"], c["tau"], c["J"], *c["drag"], CL["period"])
        b += struct.pack("<19d", *c["pos"], *c["vel"], *c["att"], *c["ang_vel"], *c["ext_force"], *c["ext_torque"])
        b += np.zeros(4, "<f4").tobytes() + np.asarray(CL_CHECKPOINTS, "<i4").tobytes() + np.ascontiguousarray(c["rows"], "<f4").tobytes()
    out = run_probe(probe, b)
    magic, n = struct.unpack_from("<2i", out, 0)
    assert magic == MAGIC_CHAIN and n == len(cases)
    off, ticks, recs = 8, [], []
    for c in cases:
        ticks.append(np.frombuffer(out, np.uint8, CL["steps"], off).copy())
        off += CL["steps"]
        recs.append(np.frombuffer(out, CL_REC, len(CL_CHECKPOINTS), off).copy())
        off += recs[-1].nbytes
    assert off == len(out) and all(np.array_equal(t, ticks[0]) for t in ticks)
    rec = np.stack(recs)
    fx = dict(dt_us=np.int32(CL["dt_us"]), period=np.float64(CL["period"]), steps=np.int32(CL["steps"]), tick=ticks[0],
              checkpoint=np.array(CL_CHECKPOINTS, np.int32), type_id=np.array([c["type_id"] for c in cases], np.int32),
              rows=np.stack([c["rows"] for c in cases]), sigma_gyro=np.float64(0.1), sigma_acc=np.float64(0.2))
    for k in PARAM_FIELDS + ("pos", "vel", "att", "ang_vel", "ext_force", "ext_torque"):
        fx["in_" + k] = np.array([c[k] for c in cases], np.float64)
    for k in CL_REC.names:
        fx["ref_" + k] = np.ascontiguousarray(rec[k])
    check_closed_loop_coverage(fx, ora)
    return fx


def check_closed_loop_coverage(fx, ora):
    n = len(fx["type_id"])
    assert n == 12 and set(fx["type_id"]) == {1, 2, 4, 5} and int(fx["steps"]) == 150
    lp = [ora.logic_params_from_type(int(t), float(fx["period"])) for t in fx["type_id"]]
    hi, lo = np.array([p.max_thrust for p in lp], np.float32), np.array([p.min_thrust for p in lp], np.float32)
    cap = np.array([p.max_cmd_total_thrust / p.mass for p in lp])
    f = fx["ref_force"]
    commanded = fx["ref_step"][0] >= fx["rows"][0, 0, 0] + 1       # checkpoints after the first tick that saw a command
    assert np.all(f[:, ~commanded] == 0) and np.all(fx["ref_cmd"][:, ~commanded] == 0)          # idle until a command arrives
    assert (f == hi[:, None, None]).any(axis=(1, 2)).sum() >= 3 and ((f == lo[:, None, None]) & commanded[None, :, None]).any(axis=(1, 2)).sum() >= 3
    assert (fx["rows"][:, :, 1] > cap[:, None]).any(axis=1).sum() >= 3                        # the total-thrust cap
    assert np.all(np.any(fx["rows"][:, 0, 1:] != fx["rows"][:, 1, 1:], axis=1) & np.any(fx["rows"][:, 1, 1:] != fx["rows"][:, 2, 1:], axis=1))
    assert (np.linalg.norm(fx["ref_ang_vel"], axis=2) * int(fx["dt_us"]) * 1e-6).max() <= SANE_TURN
    assert fx["ref_pos"][:, :, 2].min() > 1.0 and np.isfinite(fx["ref_pos"]).all()             # nobody near the ground
    assert int(fx["tick"].sum()) >= 70


def closed_loop_segments(fx):
    """[(first step, last step + 1, row handed over before the first step or -1, checkpoint reached at the end or -1)]"""
    cut = sorted(set(int(s) for s in fx["checkpoint"]) | set(int(s) - 1 for s in fx["rows"][0, :, 0]) | {int(fx["steps"])})
    cmd_at = {int(s) - 1: k for k, s in enumerate(fx["rows"][0, :, 0])}
    cp = [int(s) for s in fx["checkpoint"]]
    out, a = [], 0
    for s in cut:
        if s > a:
            out.append((a, s, cmd_at.get(a, -1), cp.index(s) if s in cp else -1))
            a = s
    return out


# ---- shared by the tests ----------------------------------------------------------------------------------------------
def load_fixture(path=FIXTURE):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def group_cases(fx, gi):
    return np.flatnonzero(fx["group"] == gi)


def group_ticks(fx, gi):
    return fx["tick"][fx["tick_offset"][gi]:fx["tick_offset"][gi + 1]]


def segments(fx, gi):
    """the rollout of a group cut where something happens: [(first step, last step + 1, command set held during them,
    checkpoint number reached at the end or -1)].  The commands of a step are those the last tick before it left
    (Quadcopter_T.cpp:98,187-189); before the first tick, set 0."""
    tick = group_ticks(fx, gi)
    steps = int(fx["group_steps"][gi])
    rows = script_rows(max(int(fx["group_ticks"][gi]), 1))
    held, runs, cp = [], 0, checkpoints(steps)
    for s in range(steps):
        held.append(0 if runs == 0 else int(rows[runs - 1]))
        runs += int(tick[s])
    out, a = [], 0
    for s in range(1, steps + 1):
        if s == steps or s in cp or held[s] != held[a]:
            out.append((a, s, held[a], cp.index(s) if s in cp else -1))
            a = s
    return out


def oracle_params(ora, fx, i):
    return ora.params_init(float(fx["in_mass"][i]), fx["in_inertia"][i], float(fx["in_arm"][i]), fx["in_com"][i], float(fx["in_min_speed"][i]),
                           float(fx["in_max_speed"][i]), float(fx["in_k_thrust"][i]), float(fx["in_k_torque"][i]), float(fx["in_tau"][i]),
                           float(fx["in_J"][i]), fx["in_drag"][i])


if __name__ == "__main__":
    if not os.path.exists(PROBE):
        sys.exit("oracle/_ref/rigid_body_probe is not built (make -C oracle ref, where the reference sources are present)")
    fixture = make_rigid_body_reference(verbose=True)
    write_fixture(make_closed_loop_reference(), CL_FIXTURE)
    print("written", CL_FIXTURE, os.path.getsize(CL_FIXTURE), "bytes")
    write_fixture(fixture)
    print("written", FIXTURE, os.path.getsize(FIXTURE), "bytes; fp32 cases %d of %d" % (fixture["fp32_ok"].sum(), len(fixture["fp32_ok"])))
