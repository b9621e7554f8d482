"""tests/golden/radio_kat.json: known answers of the REFERENCE's own radio codec (oracle/_ref/radio_probe: Common/Common/
DataTypes/RadioTypes.hpp compiled where it lies) -- all five message kinds, values at +-limit, one ulp inside it, on and one
ulp either side of half-codes (negative ones too: int(x + 0.5f) truncates toward zero), 0, -0, tiny, beyond the limit,
NaN, +-inf, and the decoding of arbitrary bytes under every type.  Floats travel as IEEE-754 bit patterns.

    python tests/golden/make_radio_kat.py     # needs oracle/_ref/radio_probe (built where the reference is)"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "radio_kat.json")
PROBE = os.path.join(ROOT, "oracle", "_ref", "radio_probe")
F = np.float32
# the limit of every float field a Create* function writes (RadioTypes.hpp:54-61,137-187)
LIMITS = {"R": (35, 35, 35, 35), "P": (20, 20, 20, 10, 10, 10, 30, 30, 30), "A": (30, 30, 30, 35)}


def edge_values(limit):
    lim = F(limit)
    inside = np.nextafter(lim, F(0))
    out = [lim, -lim, inside, -inside, np.nextafter(lim, F(np.inf)), F(1.5) * lim, F(-1.5) * lim,
           F(0), F(-0.0), F(1e-30), F(-1e-30), F(np.nan), F(np.inf), F(-np.inf)]
    for k in (0, 1, 100, 32766):
        for sign in (1, -1):
            v = F(sign * (k + 0.5) * float(lim) / 32768.0)      # scaled + 0.5f lands on or beside a whole number
            out += [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]
    return [F(v) for v in out]


def bits(v):
    return int(np.asarray(v, F).view(np.uint32))


def requests():
    rng = np.random.Generator(np.random.PCG64(20261019))
    req = []
    for op, lims in LIMITS.items():
        vals = {l: edge_values(l) for l in set(lims)}
        for k in range(max(len(v) for v in vals.values())):      # field j walks its limit's edge values, each from another start
            f = [vals[l][(k + 5 * j) % len(vals[l])] for j, l in enumerate(lims)]
            req.append(dict(op=op, flags=int(rng.integers(0, 256)), **{"in": [bits(v) for v in f]}))
        for _ in range(8):
            f = [F(rng.uniform(-1.1, 1.1) * l) for l in lims]
            req.append(dict(op=op, flags=int(rng.integers(0, 256)), **{"in": [bits(v) for v in f]}))
    for op in "KI":
        for flags in (0, 1, 2, 0x80, 0xff):
            req.append(dict(op=op, flags=flags, **{"in": []}))
    for t in (0, 1, 2, 3, 4, 5, 6, 7, 255):
        for fill in (None, 0x00, 0xff):
            raw = rng.integers(0, 256, 23) if fill is None else np.full(23, fill)
            raw[0] = t
            req.append(dict(op="D", bytes=[int(b) for b in raw]))
    return req


def run_probe(probe, req):
    lines = []
    for r in req:
        if r["op"] == "D":
            lines.append("D " + " ".join("%x" % b for b in r["bytes"]))
        else:
            lines.append("%s %x %s" % (r["op"], r["flags"], " ".join("%x" % b for b in r["in"])))
    out = subprocess.run([probe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, text=True).stdout
    ans = [json.loads(l) for l in out.splitlines()]
    assert len(ans) == len(req)
    return [dict(r, raw=a["raw"], type=a["type"], dflags=a["flags"], floats=a["floats"]) for r, a in zip(req, ans)]


def make_radio_kat(probe=PROBE):
    return dict(source="Common/Common/DataTypes/RadioTypes.hpp compiled in place (oracle/ref_radio_probe.cpp); floats are IEEE-754 bit patterns",
                limits={k: list(v) for k, v in LIMITS.items()}, cases=run_probe(probe, requests()))


def dumps(kat):
    head = {k: v for k, v in kat.items() if k != "cases"}
    return "{\n" + "".join(' %s: %s,\n' % (json.dumps(k), json.dumps(v)) for k, v in sorted(head.items())) + ' "cases": [\n' + \
        ",\n".join("  " + json.dumps(c, sort_keys=True) for c in kat["cases"]) + "\n ]\n}\n"


if __name__ == "__main__":
    if not os.path.exists(PROBE):
        sys.exit("oracle/_ref/radio_probe is not built (make -C oracle ref, where the reference sources are present)")
    with open(FIXTURE, "w") as fh:
        fh.write(dumps(make_radio_kat()))
    print("written", FIXTURE, os.path.getsize(FIXTURE), "bytes")
