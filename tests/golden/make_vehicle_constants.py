"""tests/golden/vehicle_constants.json: the REFERENCE's own type constants (oracle/_ref/constants_probe: Components/
Components/Logic/QuadcopterConstants.hpp compiled where it lies) -- for every type 0..5 every public data member its
constructor sets, and GetVehicleTypeFromID for ids 0..31.  Floats travel as IEEE-754 bit patterns ("bits"), with the
probe's decimal beside them for the reader ("decimal"; never compared).  Data only.

    python tests/golden/make_vehicle_constants.py     # needs oracle/_ref/constants_probe (built where the reference is)"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "vehicle_constants.json")
PROBE = os.path.join(ROOT, "oracle", "_ref", "constants_probe")


def make_vehicle_constants(probe=PROBE):
    out = subprocess.run([probe], stdout=subprocess.PIPE, check=True, text=True).stdout
    types = {str(t): dict(bits={}, decimal={}, ints={}) for t in range(6)}
    ids = {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "F":
            types[f[1]]["bits"][f[2]] = int(f[3], 16)
            types[f[1]]["decimal"][f[2]] = f[4]
        elif f[0] == "I":
            types[f[1]]["ints"][f[2]] = int(f[3])
        elif f[0] == "D":
            ids[int(f[1])] = int(f[2])
        else:
            raise ValueError("unexpected probe line: %r" % line)
    assert sorted(ids) == list(range(32))
    return dict(source="Components/Components/Logic/QuadcopterConstants.hpp compiled in place (oracle/ref_constants_probe.cpp); "
                       "bits are IEEE-754 float bit patterns, decimal is for the reader; members a type's branch leaves unset are absent",
                type_from_id=[ids[i] for i in range(32)], types=types)


def dumps(fx):
    lines = [' "source": %s,' % json.dumps(fx["source"]), ' "type_from_id": %s,' % json.dumps(fx["type_from_id"]), ' "types": {']
    for t in sorted(fx["types"]):
        rec = fx["types"][t]
        lines.append('  %s: {' % json.dumps(t))
        lines.append(",\n".join('   %s: %s' % (json.dumps(k), json.dumps(rec[k], sort_keys=True)) for k in sorted(rec)))
        lines.append('  }' + ("," if t != sorted(fx["types"])[-1] else ""))
    return "{\n" + "\n".join(lines) + "\n }\n}\n"


if __name__ == "__main__":
    if not os.path.exists(PROBE):
        sys.exit("oracle/_ref/constants_probe is not built (make -C oracle ref, where the reference sources are present)")
    with open(FIXTURE, "w") as fh:
        fh.write(dumps(make_vehicle_constants()))
    print("written", FIXTURE, os.path.getsize(FIXTURE), "bytes")
