"""An independent judge of RAPPIDS plans, numpy in double, written from the definitions:
the minimum-jerk primitive of Mueller, Hehn and D'Andrea (rest at the sampled point after T), its cost, thrust
|a - g| and body rate |f x j| / |f|^2 on a dense time grid, the exact per-axis speed extrema, and the distance
of the flown points to the volume a depth image shows as occupied.  It calls neither the engine nor the oracle
nor the project's root finder, and shares no code with them: what it says about a flag is a condition every
correct planner satisfies, not a restatement of how the planner decides.

Flags (DepthImagePlanner.hpp:38-44): 1 LowCost, 2 DynamicsFeasible, 4 VelocityAdmissible, 8 CollisionFree.

Also here, because the CPU and the GPU tests must draw the same thing: the aggressive distribution (samples and
states) under which all four per-candidate tests reject something.
"""
import numpy as np

LOW_COST, DYN_FEASIBLE, VEL_ADMISSIBLE, COLLISION_FREE = 1, 2, 4, 8
DENSE_POINTS = 801          # time grid of the dynamics check
CLEARANCE_POINTS = 161      # flown points judged against the image
CLEARANCE_REACH = 0.35      # [m] rays farther than this from a flown point are not looked at ...
CLEARANCE_CAP = 0.25        # ... so a clearance is reported up to here (the footprint term stays below 0.1 m)


# ---- the aggressive distribution ---------------------------------------------------------------------------------
def aggressive_samples(base_samples, seed):
    """base_samples = planner_samples(seed, W, H, n) (pixelX, pixelY, depth, duration): the pixels stay, duration
    becomes U(0.25, 3.0) s and depth U(0.6, 7.0) m -- short and far enough for thrust, body rate and speed to
    exceed their limits."""
    s = np.array(base_samples, dtype=np.float64)
    rng = np.random.default_rng(50 + seed)
    s[:, 3] = rng.uniform(0.25, 3.0, len(s))
    s[:, 2] = rng.uniform(0.6, 7.0, len(s))
    return s


def aggressive_states(seed, n, tilt_deg=35.0, upright_every=0):
    """(vel0, acc0, grav), each [3, n], camera frame (x right, y down, z forward).  Gravity is 9.81 along a unit
    vector up to tilt_deg from +y, in a random direction (pitch and roll both vary); tilt_deg = 0: exactly +y, and so
    is every upright_every-th state (the suite's other planner tests never leave +y; both must be seen)."""
    rng = np.random.default_rng(seed)
    vel0 = np.stack([rng.normal(0, 1.5, n), rng.normal(0, 1.0, n), rng.uniform(0, 5.5, n)])
    acc0 = rng.normal(0, 3.0, (3, n))
    tilt = np.radians(rng.uniform(0, tilt_deg, n))
    if upright_every:
        tilt[::upright_every] = 0.0
    azimuth = rng.uniform(0, 2 * np.pi, n)
    grav = 9.81 * np.stack([np.sin(tilt) * np.cos(azimuth), np.cos(tilt), np.sin(tilt) * np.sin(azimuth)])
    return vel0, acc0, grav


def flag_shares(flags):
    f = np.asarray(flags).ravel()
    return {v: float(np.mean(f == v)) for v in (1, 3, 7, 15)}


# ---- trajectory and cost -----------------------------------------------------------------------------------------
def end_points(cfg, samples):
    """the sampled pixel at the sampled depth, deprojected through the pinhole: [n, 3]"""
    s = np.atleast_2d(np.asarray(samples, dtype=np.float64))
    return np.stack([s[:, 2] * (s[:, 0] - cfg.cx) / cfg.focal_length, s[:, 2] * (s[:, 1] - cfg.cy) / cfg.focal_length,
                     s[:, 2]], axis=1)


def min_jerk(vel0, acc0, pf, T, with_scale=False):
    """p(t) = v0 t + a0 t^2/2 + g t^3/6 + b t^4/24 + a t^5/120 with p(T) = pf, p'(T) = p''(T) = 0: the closed form
    of the minimum-jerk problem with a fully defined end state.  vel0, acc0, pf [n, 3], T [n].
    Returns coefficients [n, 6, 3], highest power first.  with_scale: also the sum of the magnitudes of the terms each
    coefficient is the sum of -- what a rounding error of any evaluation order is relative to (a coefficient whose terms
    cancel to a thousandth of their size carries a thousand times the relative error, in every implementation)."""
    v0, a0, pf = (np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (vel0, acc0, pf))
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))[:, None]

    def three(dp, dv, da):
        return ((720.0 * dp - 360.0 * T * dv + 60.0 * T ** 2 * da) / T ** 5 / 120.0,
                (-360.0 * T * dp + 168.0 * T ** 2 * dv - 24.0 * T ** 3 * da) / T ** 5 / 24.0,
                (60.0 * T ** 2 * dp - 24.0 * T ** 3 * dv + 3.0 * T ** 4 * da) / T ** 5 / 6.0)
    c5, c4, c3 = three(pf - v0 * T - 0.5 * a0 * T ** 2, -v0 - a0 * T, -a0)
    coeffs = np.stack([c5, c4, c3, a0 / 2.0, v0, np.zeros_like(v0)], axis=1)
    if not with_scale:
        return coeffs
    s5, s4, s3 = (np.abs(x) for x in three(np.abs(pf) + np.abs(v0) * T + 0.5 * np.abs(a0) * T ** 2,
                                           -(np.abs(v0) + np.abs(a0) * T), np.abs(a0)))
    return coeffs, np.stack([s5, s4, s3, np.abs(a0) / 2.0, np.abs(v0), np.zeros_like(v0)], axis=1)


def _derivative(c, order):
    """coefficients [n, k, 3] (highest power first) of the order-th derivative"""
    c = np.asarray(c)
    for _ in range(order):
        k = c.shape[1]
        c = c[:, :-1, :] * np.arange(k - 1, 0, -1)[None, :, None]
    return c


def _evaluate(c, t):
    """polynomials [n, k, 3] at times [n, m] -> [n, m, 3]"""
    out = np.zeros(t.shape + (3,))
    for q in range(c.shape[1]):
        out = out * t[:, :, None] + c[:, q, None, :]
    return out


def costs(cfg, pf, T, cost_vec=None):
    """cost of ending at pf after T.  cost_type 0: exploration, -(direction . pf) / T; 1: progress towards a goal G,
    -(|G| - |G - pf|) / T.  cost_vec [n, 3], or None for cfg.cost_vec."""
    pf = np.atleast_2d(pf)
    T = np.atleast_1d(T)
    vec = np.array([cfg.cost_vec[0], cfg.cost_vec[1], cfg.cost_vec[2]])[None, :] if cost_vec is None else np.atleast_2d(cost_vec)
    if cfg.cost_type == 0:
        return -np.sum(vec * pf, axis=1) / T
    return -(np.linalg.norm(vec, axis=1) - np.linalg.norm(vec - pf, axis=1)) / T


# ---- dynamics and velocity ---------------------------------------------------------------------------------------
def dynamics(coeffs, grav, T, points=DENSE_POINTS):
    """(smallest thrust, largest thrust, largest body rate) over `points` times in [0, T], per trajectory.
    thrust = |a(t) - grav| [m/s^2]; body rate = |f x j| / |f|^2 with f = a - grav, j = da/dt [rad/s]."""
    coeffs = np.asarray(coeffs)
    grav = np.atleast_2d(grav)
    T = np.atleast_1d(T)
    lo, hi, rate = (np.empty(len(T)) for _ in range(3))
    acc, jerk = _derivative(coeffs, 2), _derivative(coeffs, 3)
    grid = np.linspace(0.0, 1.0, points)[None, :]

    def horner(c, t):                                    # c [n, k], t [n, m]
        out = np.zeros_like(t)
        for q in range(c.shape[1]):
            out = out * t + c[:, q, None]
        return out
    for a in range(0, len(T), 64):                        # (blocks of [64, points] doubles: they stay in cache)
        b = min(a + 64, len(T))
        t = T[a:b, None] * grid
        fx, fy, fz = (horner(acc[a:b, :, i], t) - grav[a:b, i, None] for i in range(3))
        jx, jy, jz = (horner(jerk[a:b, :, i], t) for i in range(3))
        f2 = fx * fx + fy * fy + fz * fz
        cx, cy, cz = fy * jz - fz * jy, fz * jx - fx * jz, fx * jy - fy * jx
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(f2 > 0, np.sqrt(cx * cx + cy * cy + cz * cz) / f2, np.inf)
        lo[a:b], hi[a:b], rate[a:b] = np.sqrt(f2.min(axis=1)), np.sqrt(f2.max(axis=1)), w.max(axis=1)
    return lo, hi, rate


def speed_extrema(coeffs, T):
    """max over [0, T] of |v_i(t)| per axis, exactly: the stationary points of v_i are the roots of the acceleration
    cubic (numpy.roots; the real part of a complex root is just one more time inside [0, T], which cannot exceed the
    maximum), plus both ends.  [n, 3]"""
    coeffs = np.asarray(coeffs)
    T = np.atleast_1d(T)
    vel, acc = _derivative(coeffs, 1), _derivative(coeffs, 2)
    out = np.empty((len(T), 3))
    for n in range(len(T)):
        for i in range(3):
            r = np.roots(acc[n, :, i]).real if np.any(acc[n, :, i]) else np.empty(0)
            t = np.concatenate([r[(r > 0) & (r < T[n])], [0.0, T[n]]])
            out[n, i] = np.max(np.abs(np.polyval(vel[n, :, i], t)))
    return out


def leading_sixths(coeffs):
    """|alpha| / 6 per axis, alpha = 120 c5: RapidTrajectoryGenerator.cpp:176 answers "not admissible" without looking
    at any speed when this is at most 1e-6 on an axis"""
    return np.abs(np.asarray(coeffs)[:, 0, :]) * 20.0


# ---- clearance ---------------------------------------------------------------------------------------------------
def clearance(cfg, image, coeffs, T, points=CLEARANCE_POINTS):
    """Smallest distance [m] from the flown points with z >= min_checking_dist to the occupied volume of the image, capped
    at CLEARANCE_CAP.  A pixel (x, y) with depth d = counts * depth_scale > true_vehicle_radius occupies its ray -- through
    the pixel's centre -- from depth d outward, widened by half a pixel diagonal at each depth (the pixel's footprint);
    nothing outside the image is judged.  Times are taken in groups of 16 and each group only looks at the pixels its
    points' reach can project to."""
    image = np.asarray(image)
    c = np.asarray(coeffs, dtype=np.float64).reshape(1, 6, 3)
    t = float(T) * np.linspace(0.0, 1.0, points)
    P = _evaluate(c, t[None, :])[0]
    P = P[P[:, 2] >= cfg.min_checking_dist]
    if len(P) == 0:
        return CLEARANCE_CAP
    f, m = cfg.focal_length, CLEARANCE_REACH
    near, far = np.maximum(P[:, 2] - m, 0.05), P[:, 2] + m
    # the pixel columns / rows a ball of radius m around each point can project to (x' / z' is extreme at a corner of the box)
    def span(centre, principal, size):
        cand = np.stack([(centre - m) / near, (centre - m) / far, (centre + m) / near, (centre + m) / far])
        lo = np.floor(f * cand.min(axis=0) + principal - 0.5).astype(np.int64)
        hi = np.ceil(f * cand.max(axis=0) + principal - 0.5).astype(np.int64)
        return np.clip(lo, 0, size), np.clip(hi + 1, 0, size)
    u0, u1 = span(P[:, 0], cfg.cx, cfg.width)
    v0, v1 = span(P[:, 1], cfg.cy, cfg.height)
    half_diag = np.sqrt(0.5) / f
    best = CLEARANCE_CAP
    for a in range(0, len(P), 16):
        g = slice(a, a + 16)
        xa, xb, ya, yb = u0[g].min(), u1[g].max(), v0[g].min(), v1[g].max()
        if xa >= xb or ya >= yb:
            continue
        d = image[ya:yb, xa:xb].astype(np.float64) * cfg.depth_scale
        ys, xs = np.nonzero((d > cfg.true_vehicle_radius) & (d < far[g].max()))
        if len(xs) == 0:
            continue
        d = d[ys, xs]
        ray = np.stack([(xs + xa + 0.5 - cfg.cx) / f, (ys + ya + 0.5 - cfg.cy) / f, np.ones(len(xs))], axis=1)   # z = 1: s is a depth
        rr = np.sum(ray * ray, axis=1)
        Pg = P[g]
        pr = Pg @ ray.T                                              # [times, pixels]
        s = np.maximum(pr / rr[None, :], d[None, :])                 # the nearest point of the ray at or beyond depth d
        dist2 = np.sum(Pg * Pg, axis=1)[:, None] - 2.0 * s * pr + s * s * rr[None, :]
        best = min(best, float(np.min(np.sqrt(np.maximum(dist2, 0.0)) - s * half_diag)))
    return best


# ---- the sequential search ---------------------------------------------------------------------------------------
def replay(costs_, flags):
    """FindLowestCostTrajectory's bookkeeping from the candidates' costs and flags alone: candidate k has LowCost exactly
    when its cost is below the best so far, the best moves exactly at a candidate whose flags are 15, the winner is the last
    of those.  Returns (low_cost [n] bool, best_index or -1, n_cost_checks)."""
    best, index = np.inf, -1
    low = np.zeros(len(flags), bool)
    for k, (cost, flag) in enumerate(zip(costs_, flags)):
        low[k] = cost < best
        if flag == 15:
            best, index = cost, k
    return low, index, int(low.sum())


# ---- the conditions ----------------------------------------------------------------------------------------------
class Judged:
    """everything about a set of candidates that does not depend on the limits: one per (state, sample) pair"""

    def __init__(self, cfg, vel0, acc0, grav, samples):
        self.T = np.array(np.atleast_2d(samples)[:, 3], dtype=np.float64)
        self.pf = end_points(cfg, samples)
        self.coeffs, self.coeff_scale = min_jerk(vel0, acc0, self.pf, self.T, with_scale=True)
        self.thrust_min, self.thrust_max, self.rate_max = dynamics(self.coeffs, grav, self.T)
        self.speed = speed_extrema(self.coeffs, self.T)
        self.sixths = leading_sixths(self.coeffs)


def violations(cfg, judged, flags):
    """The implications between a candidate's flags and what the judge computed; flags [n], 0 = never examined.
    Returns (list of messages -- empty for a correct planner --, measurements)."""
    flags = np.asarray(flags).ravel()
    assert len(flags) == len(judged.T)
    bad = []
    nested = np.isin(flags, (0, 1, 3, 7, 15))
    bad += ["candidate %d: flags %d do not nest" % (k, flags[k]) for k in np.flatnonzero(~nested)]
    dyn = (flags & DYN_FEASIBLE) != 0
    vel = (flags & VEL_ADMISSIBLE) != 0
    dense_ok = (judged.thrust_min >= cfg.min_thrust) & (judged.thrust_max <= cfg.max_thrust) & (judged.rate_max <= cfg.max_ang_vel)
    for k in np.flatnonzero(dyn & ~dense_ok):
        bad.append("candidate %d: called feasible with thrust %.4f .. %.4f, body rate %.4f" %
                   (k, judged.thrust_min[k], judged.thrust_max[k], judged.rate_max[k]))
    top = judged.speed.max(axis=1)
    for k in np.flatnonzero(vel & ~(top < cfg.max_velocity)):
        bad.append("candidate %d: called admissible with an axis at %.6f m/s" % (k, top[k]))
    early = (judged.sixths <= 1e-6).any(axis=1)
    for k in np.flatnonzero(dyn & ~vel & ~(top >= cfg.max_velocity) & ~early):
        bad.append("candidate %d: called too fast at %.6f m/s" % (k, top[k]))
    rejected = ((flags & LOW_COST) != 0) & ~dyn
    seen = {"candidates": int(len(flags)),
            "accepted_thrust_min": float(judged.thrust_min[dyn].min()) if dyn.any() else None,
            "accepted_thrust_max": float(judged.thrust_max[dyn].max()) if dyn.any() else None,
            "accepted_body_rate_max": float(judged.rate_max[dyn].max()) if dyn.any() else None,
            "accepted_speed_max": float(top[vel].max()) if vel.any() else None,
            "rejected_speed_min": float(top[dyn & ~vel & ~early].min()) if (dyn & ~vel & ~early).any() else None,
            "dynamics_rejected": int(rejected.sum()),
            "dynamics_rejected_but_dense_feasible": int((rejected & dense_ok).sum())}
    return bad, seen


def winner_violations(cfg, image, judged, k, coeffs, best_cost, cost):
    """a plan's winner, candidate k of `judged`: its polynomial is the closed form (to 1e-12 of the terms each coefficient
    sums, see min_jerk), its cost the judge's (1e-13) and it stays clear of the image by the vehicle's radius.
    Returns (messages, clearance)."""
    bad = []
    got, want = np.asarray(coeffs, dtype=np.float64).reshape(6, 3), judged.coeffs[k]
    if not np.all(np.abs(got - want) <= 1e-12 * judged.coeff_scale[k]):
        bad.append("winner %d: coefficients off by %.3g relative" % (k, np.max(np.abs(got - want) / np.maximum(judged.coeff_scale[k], 1e-300))))
    if not abs(best_cost - cost) <= 1e-13 * max(1.0, abs(cost)):
        bad.append("winner %d: cost %.17g, judge %.17g" % (k, best_cost, cost))
    clear = clearance(cfg, image, got, judged.T[k])
    if not clear >= cfg.true_vehicle_radius:
        bad.append("winner %d: called collision-free %.4f m from an obstacle" % (k, clear))
    return bad, clear


def merge_seen(total, seen):
    """fold one violations() measurement into a running one"""
    if not total:
        return dict(seen)
    out = dict(total)
    for key, value in seen.items():
        if key in ("candidates", "dynamics_rejected", "dynamics_rejected_but_dense_feasible"):
            out[key] = total[key] + value
        elif value is not None:
            pick = min if key.endswith("_min") else max
            out[key] = value if total[key] is None else pick(total[key], value)
    return out
