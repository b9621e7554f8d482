"""The step kernels as a finite matrix, stated once (plain module: no fixtures, no GPU needed to import it).

run_vehicle (agri-fly_amd/csrc/afe_kernels.hip) is compiled into one kernel per combination of template flags, in four
kernel templates; launch_step / launch_persistent pick one at run time from the engine's configuration.  Here:

  cells()                 every variant the dispatch macros instantiate, as Cell records
  cell_of(mangled_name)   a kernel symbol of the code object -> its Cell  (tests/test_step_matrix_cpu.py: the two are one set)
  configure(afa, c, d)    an engine that will launch exactly that variant, with the reaching asserted before it steps
  fly / oracle_run        one flight of the engine, the double-precision oracle of the same configuration

tests/test_gpu_step_matrix.py flies every cell once on purpose."""
import collections
import re
import types as _types

import numpy as np

Cell = collections.namedtuple("Cell", "family precision fext text noise logic buf cp resident")
# family     args_single | args_fused (afe_step_kernel<.., SINGLE, ..>: the record in the kernel arguments), wave_types
#            (afe_step_kernel_wave_types: one scalar-loaded record per wave), table (afe_step_kernel_table: table in LDS),
#            grid (afe_step_persistent_kernel: the resident grid)
# precision  "f32" | "f64";  fext, text, logic, buf: bool;  noise: 0 off, 1 libstdc++ streams, 2 counter
# cp         args_single only (else None): the cache policy 0..3; 1..3 exist only with buf and without text
# resident   grid only (else None); grids have no text and always address through buffer resources

FAMILIES = ("args_single", "args_fused", "wave_types", "table", "grid")
PRECISIONS = ("f32", "f64")

# a cell the C ABI cannot reach would be listed here with the reason from the dispatch code (and still be a cell: the
# completeness test counts it, the flights skip it).  There is none: every instantiation of launch_step /
# launch_persistent hangs on run-time flags an engine can be given (afe_engine.cpp afe_step, persist_flags).
UNREACHABLE = {}


def cells():
    out = []
    tf = (False, True)
    for precision in PRECISIONS:
        for fext in tf:
            for noise in (0, 1, 2):
                for logic in tf:
                    for text in tf:
                        for buf in tf:
                            for cp in (0, 1, 2, 3):
                                if cp == 0 or (buf and not text):         # launch_step: CPOK = BU && !TE, else the default kernel
                                    out.append(Cell("args_single", precision, fext, text, noise, logic, buf, cp, None))
                            for family in ("args_fused", "wave_types", "table"):
                                out.append(Cell(family, precision, fext, text, noise, logic, buf, None, None))
                    for resident in tf:
                        out.append(Cell("grid", precision, fext, False, noise, logic, True, None, resident))
    return out


def key(c):
    s = "%s/%s/F%dT%dN%dL%dB%d" % (c.family, c.precision, c.fext, c.text, c.noise, c.logic, c.buf)
    if c.cp is not None:
        s += "/cp%d" % c.cp
    if c.resident is not None:
        s += "/res%d" % c.resident
    return s


_TEMPLATES = ("afe_step_kernel", "afe_step_kernel_wave_types", "afe_step_kernel_table", "afe_step_persistent_kernel")


def _function_name(mangled_name):
    """(the function's own name, what follows it) of an Itanium-mangled symbol, namespaces skipped: _ZN3afe15afe_step_kernelI..."""
    m = re.match(r"^_ZN?", mangled_name)
    if not m:
        return None, ""
    at, name = m.end(), None
    while True:
        m = re.compile(r"\d+").match(mangled_name, at)
        if not m:
            return name, mangled_name[at:]
        at = m.end() + int(m.group())
        name = mangled_name[m.end():at]


def is_step_kernel(mangled_name):
    """every kernel whose name says it steps vehicles -- a fifth template would be one, and cell_of refuses it"""
    name, _ = _function_name(mangled_name)
    return name is not None and re.match(r"^afe_step_\w*kernel", name) is not None


def cell_of(mangled_name):
    """_ZN3afe15afe_step_kernelIfLb1ELb0ELi2ELb0ELb1ELb1ELi0EEEv... -> Cell; ValueError for anything that is not one of the
    four templates with exactly the template arguments this module knows (a new flag, a new template)"""
    template, rest = _function_name(mangled_name)
    m = re.match(r"^I([fd])((?:L[bi]\d+E)*)E", rest)
    if template not in _TEMPLATES or not m:
        raise ValueError("not a step kernel of a known template: " + mangled_name)
    real, arg_text = m.groups()
    args = [(kind, int(val)) for kind, val in re.findall(r"L([bi])(\d+)E", arg_text)]
    kinds = "".join(k for k, _ in args)
    vals = [v for _, v in args]
    precision = "f32" if real == "f" else "f64"
    want = {"afe_step_kernel": "bbibbbi", "afe_step_kernel_wave_types": "bbibb", "afe_step_kernel_table": "bbibb",
            "afe_step_persistent_kernel": "bibb"}[template]
    if kinds != want:
        raise ValueError("template arguments %r of %s are not the %r this matrix knows: %s" % (kinds, template, want, mangled_name))
    if template == "afe_step_kernel":
        fext, text, noise, logic, single, buf, cp = vals
        if not single and cp != 0:
            raise ValueError("a fused launch with a cache policy: " + mangled_name)
        return Cell("args_single" if single else "args_fused", precision, bool(fext), bool(text), noise, bool(logic), bool(buf),
                    cp if single else None, None)
    if template == "afe_step_persistent_kernel":
        fext, noise, logic, resident = vals
        return Cell("grid", precision, bool(fext), False, noise, bool(logic), True, None, bool(resident))
    fext, text, noise, logic, buf = vals
    return Cell("wave_types" if template.endswith("wave_types") else "table", precision, bool(fext), bool(text), noise,
                bool(logic), bool(buf), None, None)


# ---------------------------------------------------------------------------------------------------------------------
# shapes and inputs

N_SMALL = 325            # five full waves and a ragged sixth; two workgroups of the 256-thread table kernel
N_XCD = 1024             # cp == 3: sixteen one-wave workgroups, the smallest grid on which the per-XCD remap is no identity
FIRST_GLOBAL = 1_000_003
DT_US, PERIOD, STEPS = 1000, 1 / 500, 12
SIGMA_GYRO, SIGMA_ACC = 0.1, 0.2
NOISE_SEED = 0x5eed0c0ffee12345
TYPE_IDS = (5, 1, 2, 4)
TABLES = ("shipped", "modified")


def n_of(c):
    return N_XCD if c.cp == 3 else N_SMALL


def layout_of(c):
    return {"wave_types": "by_wave", "table": "random"}.get(c.family, "record0")


def script_of(c):
    """[[calls before the command], [calls under the command], [calls after the partial re-command]] -- n_steps per
    afe_step call, 12 steps in all.  Without logic the three parts are simply flown one after the other."""
    if c.family == "args_single":
        return [[1, 1], [1] * 5, [1] * 5]
    if c.family == "grid":
        return [[1, 1], [1], [9]]                       # three single-step calls, then nine steps in one
    # fused launches: 7 + 5 (both calls hold ticks, the odd split moves the tick's bit in the mask, tick_base is carried);
    # with logic the two idle steps are a call of their own and 7 + 3 follow
    return [[2], [7], [3]] if c.logic else [[], [7], [5]]


def _oracle_params(ora, p):
    return ora.params_init(p.mass, list(p.inertia), p.arm_length, list(p.com_error), p.motor_min_speed, p.motor_max_speed,
                           p.prop_thrust_from_speed_sqr, p.prop_torque_from_speed_sqr, p.motor_time_const, p.motor_inertia,
                           list(p.lin_drag_coeff_b), (p.imu_yaw, p.imu_pitch, p.imu_roll))


def type_table(afa, ora, kind):
    """(engine records, oracle records).  shipped: types 5, 1, 2, 4 as they are (stateless motors, identity mount).
    modified: the recipe of tests/campaigns/step_campaign.py random_table with a fixed seed, every family of change
    present in EVERY record (the record-0 layouts see record 0 only): lagged rotor with inertia, CoM error, drag, a full
    inertia tensor, a tilted IMU mount."""
    plist = [afa.params_from_type(t) for t in TYPE_IDS]
    if kind == "modified":
        rng = np.random.default_rng(20260)
        for p in plist:
            p.mass *= float(rng.uniform(0.8, 1.25))
            p.motor_time_const = float(rng.uniform(0.008, 0.06))
            p.motor_inertia = float(rng.uniform(1e-8, 2e-6))
            for k in range(3):
                p.com_error[k] = float(rng.normal(0, 1.5e-3))
                p.lin_drag_coeff_b[k] = float(rng.uniform(0.02, 0.3))
            A = rng.normal(size=(3, 3)) * 0.15
            I = np.array(p.inertia).reshape(3, 3)
            I = I + A @ A.T * I[0, 0]
            for a in range(9):
                p.inertia[a] = float(I.reshape(9)[a])
            p.imu_yaw, p.imu_pitch, p.imu_roll = [float(x) for x in rng.uniform(-0.6, 0.6, 3)]
    else:
        assert kind == "shipped"
    return plist, [_oracle_params(ora, p) for p in plist]


def flight_data(afa, ora, table, layout, n):
    """everything a flight and its oracle start from, seeded by (table, layout, n)"""
    d = _types.SimpleNamespace(table=table, layout=layout, n=n, first_global=FIRST_GLOBAL)
    rng = np.random.default_rng([7, TABLES.index(table), ("record0", "by_wave", "random").index(layout), n])
    d.plist, d.olist = type_table(afa, ora, table)
    d.lagged = any(p.motor_time_const > 0 or p.motor_inertia > 0 for p in d.plist)
    nt = len(TYPE_IDS)
    if layout == "record0":
        d.types = np.zeros(n, np.uint8)
    elif layout == "by_wave":       # constant over aligned runs of 64, three types and more, the ragged tail a type of its own
        waves = (n + 63) // 64
        per_wave = np.array([(1 + w) % (nt - 1) for w in range(waves - 1)] + [nt - 1], np.uint8)
        d.types = per_wave[np.arange(n) // 64]
        assert len(set(per_wave.tolist())) >= 3 and (per_wave[:-1] != per_wave[-1]).all() and n % 64
    else:
        d.types = rng.integers(0, nt, n).astype(np.uint8)
        assert len(set(d.types[:64].tolist())) > 1
    ens = afa.scenarios.random_ensemble(n, int(rng.integers(1 << 30)), type_ids=TYPE_IDS, ground_fraction=0.0)
    ens.pos[2] += 40                                                      # room to fall, as the campaigns do
    d.pos, d.vel, d.att, d.ang_vel = ens.pos, ens.vel, ens.att, ens.ang_vel * 0.3
    d.ext_force, d.ext_torque = ens.ext_force, ens.ext_torque
    wmax = np.array([p.motor_max_speed for p in d.plist])[d.types]
    hover = np.array([p.hover_speed for p in d.plist])[d.types]
    # open loop: commands with a few above the clamp and a few negative, rotor speeds anywhere below the maximum but not 0
    d.cmd = (rng.uniform(0, 1.05, (4, n)) * wmax).astype(np.float32)
    d.cmd[0, rng.random(n) < 0.03] = -50.0
    d.speed = rng.uniform(0.05, 1, (4, n)) * wmax
    assert (d.cmd > wmax).any() and (d.cmd < 0).any() and (d.speed > 0).all()
    # closed loop (run_logic_campaign): rotors near hover, no commands until the logic writes them, thrust up to saturation
    d.speed_logic = hover * (1 + 0.05 * rng.uniform(-0.5, 0.5, (4, n)))
    d.thrust = np.clip(9.81 + rng.normal(0, 3.0, n), 0, 25).astype(np.float32)
    d.wdes = rng.normal(0, 2.0, (3, n)).astype(np.float32)
    d.thrust_b = np.clip(9.81 + rng.normal(0, 1.0, n), 0, 25).astype(np.float32)
    d.wdes_b = rng.normal(0, 0.5, (3, n)).astype(np.float32)
    d.half = n // 2
    d.ticks = afa.plan_ticks(PERIOD, 0, DT_US, STEPS)[0]
    assert d.ticks.sum() >= 4
    return d


# ---------------------------------------------------------------------------------------------------------------------
# the engine side

def configure(afa, c, d):
    """an engine that will launch exactly the kernel of cell c on the inputs d; what can be known before the first step
    is asserted here, what only a step shows (a resident grid that is running) in fly()"""
    assert c not in UNREACHABLE, UNREACHABLE.get(c)
    assert d.n == n_of(c) and d.layout == layout_of(c)
    e = afa.Ensemble(d.n, precision=afa.AFE_F32 if c.precision == "f32" else afa.AFE_F64, first_global_index=d.first_global)
    try:
        e.set_type_table(d.plist)
        e.set_vehicle_types(d.types)
        e.set_logic_period(PERIOD)
        e.set_addressing(not c.buf)
        e.set_cache_policy(c.cp or 0)
        e.set_step_mode({None: afa.AFE_STEP_LAUNCH, False: afa.AFE_STEP_PERSISTENT, True: afa.AFE_STEP_RESIDENT}[c.resident])
        e.set_split_stepping(1)
        e.set_max_fused_steps(1 if c.family == "args_single" else 8)
        e.set_imu_noise(c.noise != 0, SIGMA_GYRO, SIGMA_ACC, afa.AFE_SEED_COUNTER if c.noise == 2 else afa.AFE_SEED_DECORRELATED)
        e.set_noise_seed(NOISE_SEED)
        e.set_state(d.pos, d.vel, d.att, d.ang_vel, d.speed_logic if c.logic else d.speed)
        e.set_motor_cmds(np.zeros((4, d.n), np.float32) if c.logic else d.cmd)
        if c.fext:
            e.set_external_force(d.ext_force)
        if c.text:
            e.set_external_torque(d.ext_torque)
        if c.logic:
            e.set_rates_logic([afa.rates_logic_params_from_type(t) for t in TYPE_IDS])
        want_path = {"record0": "kernel arguments", "by_wave": "per-wave scalar loads", "random": "LDS table"}[d.layout]
        assert e.step_kernel_info() == (want_path, "buffer" if c.buf else "global"), (key(c), e.step_kernel_info())
        assert e.cache_policy_in_use == (c.cp or 0), (key(c), e.cache_policy_in_use)
        if c.cp == 3:
            assert ((d.n + 63) // 64) % 8 == 0 and (d.n + 63) // 64 > 8     # else the host demotes it to 2 / the remap is the identity
    except BaseException:
        e.close()
        raise
    return e


def fly(afa, c, d, export_view=False):
    """configure, fly the cell's script, read everything back; the engine is closed (a resident grid parked) on return.
    export_view: take device_view() first -- an fp32 one-step grid then reads its inputs from memory, not from LDS."""
    e = configure(afa, c, d)
    try:
        if export_view:
            e.device_view()
        rng0 = e.get_rng_state()
        first = True
        for part, calls in enumerate(script_of(c)):
            if c.logic and part == 1:
                e.set_rates_commands(d.thrust, d.wdes)
            if c.logic and part == 2:
                e.set_rates_commands(d.thrust_b[:d.half], d.wdes_b[:, :d.half], first=0, count=d.half)
            for k in calls:
                e.step(DT_US, k)
                if first and c.family == "grid":
                    # the persistent mode falls back to launches silently, and a cell that fell back has not been flown
                    assert e.persistent_running, key(c) + ": the resident grid did not start"
                first = False
        got = e.get_state()
        got["gyro"], got["acc"] = e.get_imu()
        got["motor_cmd"] = e.get_motor_cmds()
        got["rng"], got["rng0"] = e.get_rng_state(), rng0
        got["logic_ticks"], got["time_us"] = e.logic_ticks, e.time_us
    finally:
        e.close()
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the oracle side

def oracle_key(c, d):
    """what an oracle run depends on: not the precision, the addressing, the cache policy or how the steps are grouped into
    calls -- only (with logic) on where the commands fall"""
    parts = tuple(sum(p) for p in script_of(c)) if c.logic else None
    return (c.fext, c.text, c.noise, c.logic, d.layout, d.table, d.n, parts)


def oracle_run(ora, c, d, rng0):
    olist = []
    for o in d.olist:
        q = ora.OraParams.from_buffer_copy(o)
        q.sigma_gyro, q.sigma_acc = (SIGMA_GYRO, SIGMA_ACC) if c.noise else (0.0, 0.0)
        olist.append(q)
    b = ora.Batch(d.n, olist, d.types)
    b.pos[:], b.vel[:], b.att[:], b.ang_vel[:] = d.pos, d.vel, d.att, d.ang_vel
    b.motor_speed[:] = d.speed_logic if c.logic else d.speed
    b.motor_cmd[:] = 0 if c.logic else d.cmd
    if c.fext:
        b.ext_force[:] = d.ext_force
    if c.text:
        b.ext_torque[:] = d.ext_torque
    if c.noise == 1:
        b.rng[:] = rng0
    counter = dict(seed=NOISE_SEED, first_global=d.first_global)
    dt = DT_US * 1e-6
    if not c.logic:
        if c.noise == 2:
            ora.step_counter(b, DT_US, STEPS, d.ticks, counter_noise=True, **counter)
        else:
            b.step(dt, STEPS, ticks=d.ticks)
        return b
    k0, k1, k2 = (sum(p) for p in script_of(c))
    cl = ora.ClosedLoopBatch(b, [ora.logic_params_from_type(t, PERIOD) for t in TYPE_IDS], PERIOD,
                             counter=counter if c.noise == 2 else None)
    cl.step(dt, d.ticks[:k0])
    cl.set_rates_cmd(d.thrust, d.wdes)
    cl.step(dt, d.ticks[k0:k0 + k1])
    t2, w2 = d.thrust.copy(), d.wdes.copy()
    t2[:d.half], w2[:, :d.half] = d.thrust_b[:d.half], d.wdes_b[:, :d.half]
    cl.set_rates_cmd(t2, w2)
    cl.step(dt, d.ticks[k0 + k1:])
    assert k0 + k1 + k2 == STEPS
    return b
