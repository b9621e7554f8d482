"""Talking to oracle/_ref/gps_probe, the reference's own Offboard::GPSIMUStateEstimator compiled where it lies against the
recording dense stand-in oracle/eigen_dense (test infrastructure; the protocol is written at the head of
oracle/ref_gps_probe.cpp, and what may be concluded from the numbers at the head of oracle/eigen_dense/Eigen/Dense).
Nothing here computes a number of the estimator.

  Request            the call list: clock, new, load, write, predict, update, reset (every double as a hex float: bit for bit)
  run_probe          one child process on the CPU -> [block per answered call]
  fly(script, inputs, n, teacher=None)
                     a script of tests/gps_estimator_checker.py (make_script, make_phase_script, ...) with the inputs of
                     synthetic_inputs, vehicle by vehicle, call for call what gps_estimator_checker.run_script hands the
                     definition.  teacher: the definition's state BEFORE every event (run_script's states, shifted by one, with
                     `corr`); it is loaded in front of every call, so that differences of evaluation order cannot pile up.
                     -> blocks[event][vehicle] (None where the event makes no call for that vehicle)"""
import os
import subprocess

import numpy as np

from tests import gps_estimator_checker as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "oracle", "_ref", "gps_probe")
PRODUCT, DETERMINANT, INVERSE = 0, 1, 2
BRANCHES = ("constructed", "reset", "first_predict", "predict", "measure_before_predict", "singular", "update")


def _hex(values):
    return " ".join(float(x).hex() for x in values)


class Request:
    def __init__(self):
        self.lines, self.answered = [], 0

    def clock(self, us):
        self.lines.append("C %d" % int(us))

    def new(self, vid):
        self.lines.append("N %d" % vid)
        self.answered += 1

    def load(self, vid, initialized, num_resets, t_predict, t_update, est13, corr3, cov81):
        self.lines.append("L %d %d %d %d %d %s %s %s" % (vid, int(initialized), int(num_resets), int(t_predict), int(t_update), _hex(est13),
                                                        _hex(corr3), _hex(cov81)))

    def write(self, vid, est13, corr3, cov81):
        self.lines.append("W %d %s %s %s" % (vid, _hex(est13), _hex(corr3), _hex(cov81)))

    def predict(self, vid, acc, gyro):
        self.lines.append("P %d %s %s" % (vid, _hex(acc), _hex(gyro)))
        self.answered += 1

    def update(self, vid, pos):
        self.lines.append("U %d %s" % (vid, _hex(pos)))
        self.answered += 1

    def reset(self, vid):
        self.lines.append("R %d" % vid)
        self.answered += 1

    def bytes(self):
        return ("\n".join(self.lines) + "\n").encode()


def _floats(tokens):
    return np.array([float.fromhex(t) for t in tokens], np.float64)


def parse(answer, n_blocks):
    blocks, cur = [], None
    lines = answer.decode().split("\n")
    k = 0
    while k < len(lines):
        t = lines[k].split()
        k += 1
        if not t:
            continue
        if t[0] == "S":
            f = _floats(t[6:])
            assert f.size == 20 + 81, f.size
            cur = dict(id=int(t[1]), initialized=int(t[2]), num_resets=int(t[3]), last_predict_us=int(t[4]), last_update_us=int(t[5]), est=f[0:13],
                       corr=f[13:16], last_meas_att=f[16:20], cov=f[20:], tape=[])
        elif t[0] == "B":
            cur["branch"] = t[1]
        elif t[0] == "T":
            kind, r, kk, c = (int(x) for x in t[1:5])
            a, b, o = (lines[k + i].split() for i in range(3))
            k += 3
            assert (a[0], b[0], o[0]) == ("A", "B", "O")
            cur["tape"].append(dict(kind=kind, r=r, k=kk, c=c, a=_floats(a[1:]), b=_floats(b[1:]), out=_floats(o[1:])))
        elif t[0] == "E":
            blocks.append(cur)
            cur = None
        else:
            raise AssertionError("oracle/_ref/gps_probe wrote %r" % lines[k - 1][:80])
    assert cur is None and len(blocks) == n_blocks, (len(blocks), n_blocks)
    return blocks


def run_probe(request, probe=PROBE):
    """the reference prints its own line to stderr in the singular branch (:229); it is dropped"""
    out = subprocess.run([probe], input=request.bytes(), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    assert out.returncode == 0, "oracle/_ref/gps_probe ended with status %r" % out.returncode
    return parse(out.stdout, request.answered)


def fly(script, inputs, n, teacher=None, probe=PROBE):
    req = Request()
    req.clock(0)
    for v in range(n):
        req.new(v)
    where = []                                    # per event: {vehicle: index of its block}
    made = n

    def call(ev_calls, v):
        nonlocal made
        ev_calls[v] = made
        made += 1

    for k, ev in enumerate(script):
        calls = {}
        if teacher is not None and ev[0] in ("imu", "measure", "reset", "reset_ranges"):
            st = teacher[k]
            for v in range(n):
                req.load(v, st["initialized"][v], st["num_resets"][v], st["last_predict_us"][v], st["last_update_us"][v], st["est"][:, v],
                         st["corr"][:, v], st["cov"][:, v])
        if ev[0] == "imu":
            now, a, w = inputs[k]
            req.clock(now)
            for v in range(n):
                req.predict(v, a[:, v], w[:, v])
                call(calls, v)
        elif ev[0] == "measure":
            now, z = inputs[k]
            req.clock(now)
            for v in range(n):
                req.update(v, z[:, v])
                call(calls, v)
        elif ev[0] in ("reset", "reset_ranges"):
            req.clock(inputs[k])
            for first, count in ([(ev[1], ev[2])] if ev[0] == "reset" else ev[1]):
                for v in range(first, first + count):
                    req.reset(v)
                    call(calls, v)
        else:                                      # set_state: the float members written, _initialized set
            e13, c81, k3 = gc.payload(ev[1], ev[3], inputs[k])
            for i in range(ev[3]):
                req.write(ev[2] + i, e13[:, i], k3[:, i], c81[:, i])
        where.append(calls)
    blocks = run_probe(req, probe)
    return [{v: blocks[i] for v, i in calls.items()} for calls in where], blocks[:n]
