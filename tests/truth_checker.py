"""The depth-image ground truth (DepthImagePlanner.cpp:1031-1098, IsCollisionFreeGroundTruth) restated in numpy float64,
operation for operation as agri-fly_amd/csrc/afe_truth.hip states it, visiting EVERY pixel of the image: the judge of the
device kernel, which scans only the rectangle that bounds the sphere's image.  Test infrastructure; no GPU.

Everything is IEEE double; numpy's + - * / and sqrt are correctly rounded, Python evaluates a*b*c left to right.

    sample times   t_0 = t_begin, t_{k+1} = t_k + timestep while t_k < t_end (running sum);  K > 4096 is refused
    position       c0*t*t*t*t*t + c1*t*t*t*t + c2*t*t*t + c3*t*t + c4*t + c5 per axis
    scalars        ignore = uint16(true_vehicle_radius / depth_scale), edge = int(f * true_vehicle_radius / min_checking_dist)
    skipped        p.z < min_checking_dist (a NaN is not skipped), in both passes
    field of view  px = p.x*f/p.z + cx, py likewise;  px <= edge or px > W - edge or py <= edge or py > H - edge: verdict 1
    pixels         depth > ignore:  ex = (x - cx)/f, ey = (y - cy)/f, n = float32(sqrt(ex*ex + ey*ey + 1.0*1.0)),
                   u = (ex/n, ey/n, 1.0/n), d = p.x*u.x + p.y*u.y + p.z*u.z, s = d*d - (p.x*p.x + p.y*p.y + p.z*p.z) + r*r;
                   s >= 0 and sqrt(q.q) < d + sqrt(s) with q = (m*ex, m*ey, m*1.0), m = depth*depth_scale: verdict 2
"""
import numpy as np

MAX_SAMPLES = 4096
RECORD_FIELDS = ("verdict", "k_fov", "t_fov", "k_hit", "t_hit", "pixel_hit", "n_samples", "n_checked")
EMPTY_RECORD = dict(verdict=-1, k_fov=-1, t_fov=float("nan"), k_hit=-1, t_hit=float("nan"), pixel_hit=-1, n_samples=0, n_checked=0)


def sample_times(t_begin, t_end, timestep):
    """the running sum; None when there would be more than 4096 samples"""
    assert np.isfinite(timestep) and timestep > 0
    out, t = [], float(t_begin)
    while t < t_end:
        if len(out) == MAX_SAMPLES:
            return None
        out.append(t)
        t = t + float(timestep)
    return out


def position(coeffs, t):
    """coeffs [6][3] -> (x, y, z) by the power form"""
    c = coeffs
    return tuple(float(c[0][a]) * t * t * t * t * t + float(c[1][a]) * t * t * t * t + float(c[2][a]) * t * t * t +
                 float(c[3][a]) * t * t + float(c[4][a]) * t + float(c[5][a]) for a in range(3))


def scalars(cfg):
    """(ignore, edge), or None where the truncations are not defined (the library refuses those)"""
    if not cfg.min_checking_dist > 0:
        return None
    with np.errstate(all="ignore"):
        qi = np.float64(cfg.true_vehicle_radius) / np.float64(cfg.depth_scale)
        qe = np.float64(cfg.focal_length) * np.float64(cfg.true_vehicle_radius) / np.float64(cfg.min_checking_dist)
    if not (-1.0 < qi < 65536.0) or not (-2.0 ** 30 < qe < 2.0 ** 30):
        return None
    return int(qi), int(qe)


class ImageRays:
    """What depends on the image and the configuration alone, formed once per image: the definition's ex, ey, u and the
    distance sqrt(q.q) of every pixel, and which pixels are deeper than `ignore`."""

    def __init__(self, cfg, depth):
        depth = np.asarray(depth)
        assert depth.shape == (cfg.height, cfg.width)
        self.cfg = cfg
        self.ignore, self.edge = scalars(cfg)
        f = np.float64(cfg.focal_length)
        x = np.arange(cfg.width, dtype=np.float64)[None, :]
        y = np.arange(cfg.height, dtype=np.float64)[:, None]
        ex = np.broadcast_to((x - np.float64(cfg.cx)) / f, depth.shape)
        ey = np.broadcast_to((y - np.float64(cfg.cy)) / f, depth.shape)
        n = np.sqrt(ex * ex + ey * ey + 1.0 * 1.0).astype(np.float32).astype(np.float64)
        self.seen = (depth.astype(np.int64) > self.ignore).reshape(-1)
        self.ux, self.uy, self.uz = (ex / n).reshape(-1), (ey / n).reshape(-1), (1.0 / n).reshape(-1)
        m = depth.astype(np.float64) * np.float64(cfg.depth_scale)
        qx, qy, qz = m * ex, m * ey, m * 1.0
        self.dist = np.sqrt(qx * qx + qy * qy + qz * qz).reshape(-1)

    def first_occluding_pixel(self, p):
        """the lowest y*W + x whose pixel occludes the sphere at p, or -1"""
        px, py, pz = (np.float64(v) for v in p)
        r = np.float64(self.cfg.planning_vehicle_radius)
        with np.errstate(all="ignore"):
            d = px * self.ux + py * self.uy + pz * self.uz
            s = d * d - (px * px + py * py + pz * pz) + r * r
            meets = self.seen & (s >= 0)
            hit = np.zeros(len(d), bool)
            hit[meets] = self.dist[meets] < d[meets] + np.sqrt(s[meets])
        at = np.flatnonzero(hit)
        return int(at[0]) if len(at) else -1


def judge(rays, coeffs, t_begin, t_end, timestep=0.1):
    """one path against one image (an ImageRays) -> the record as a dict of RECORD_FIELDS"""
    cfg = rays.cfg
    times = sample_times(t_begin, t_end, timestep)
    assert times is not None, "more than 4096 samples"
    rec = dict(EMPTY_RECORD, verdict=0, n_samples=len(times))
    f, cx, cy, near = float(cfg.focal_length), float(cfg.cx), float(cfg.cy), float(cfg.min_checking_dist)
    right, bottom = cfg.width - rays.edge, cfg.height - rays.edge
    points = [position(coeffs, t) for t in times]
    with np.errstate(all="ignore"):
        for k, p in enumerate(points):
            if p[2] < near:
                continue
            ix = np.float64(p[0]) * f / np.float64(p[2]) + cx
            iy = np.float64(p[1]) * f / np.float64(p[2]) + cy
            if ix <= rays.edge or ix > right or iy <= rays.edge or iy > bottom:
                rec.update(verdict=1, k_fov=k, t_fov=times[k])
                return rec
    for k, p in enumerate(points):
        if p[2] < near:
            continue
        rec["n_checked"] += 1
        pixel = rays.first_occluding_pixel(p)
        if pixel >= 0:
            rec.update(verdict=2, k_hit=k, t_hit=times[k], pixel_hit=pixel)
            return rec
    return rec


def judge_batch(cfg, images, coeffs, t_range, image_index=None, timestep=0.1):
    """n paths (coeffs [n, 6, 3], t_range [2, n]) -> list of records; image_index[i] (default i) names path i's image"""
    rays = {}
    out = []
    for i in range(len(coeffs)):
        j = i if image_index is None else int(image_index[i])
        if j not in rays:
            rays[j] = ImageRays(cfg, images[j])
        out.append(judge(rays[j], coeffs[i], t_range[0][i], t_range[1][i], timestep))
    return out


def records_equal(device, want):
    """every field of every record, NaN equal to NaN; returns the list of differences"""
    bad = []
    for i, w in enumerate(want):
        for name in RECORD_FIELDS:
            a, b = device[name][i], w[name]
            same = (np.isnan(a) and np.isnan(b)) if isinstance(b, float) else int(a) == int(b)
            if not same and not (isinstance(b, float) and float(a) == b):
                bad.append((i, name, a.item(), b))
    return bad


def tally(flags, verdicts):
    """MeasureConservativeness' counts from the planner's flags and the verdicts (any shape) -> dict"""
    fl, v = np.asarray(flags).reshape(-1), np.asarray(verdicts).reshape(-1)
    checked = (fl & 4) != 0
    free = checked & ((fl & 8) != 0)
    collides = checked & ~free
    return dict(n_checked=int(checked.sum()), n_planner_free=int(free.sum()),
                n_correct_in_collision=int((collides & (v != 0)).sum()), n_incorrect_in_collision=int((collides & (v == 0)).sum()),
                n_free_but_out_of_view=int((free & (v == 1)).sum()), n_free_but_occluded=int((free & (v == 2)).sum()))
