"""The drop-in branch meets the reference's own headers (round-4 review, "What's missing" 3).

include/agrifly/SimulationObject6DOF.hpp and Quadcopter_T.hpp have two faces: outside the agri-fly tree they bring
stand-alone look-alikes of the Vehicle API (standalone_types.hpp -- what every other test compiles against); INSIDE
the tree (-DAGRIFLY_USE_REFERENCE_TYPES) they forward to the tree's Components/Simulation/SimulationObject6DOF.hpp and
agrifly::Quadcopter_T derives from THE Simulation::SimulationObject6DOF.  That second face is what INTEGRATION.md
section 2 tells a maintainer to build.

The compiling is done by build(), through the committed recipe oracle/Makefile (`make ref`, where the agri-fly tree is
present at build time -- REF): tests/cpp/dropin_reference_types.cpp -- the vehicle of Simulator/Rappids_Simulator/
main.cpp:146-218, same fifteen constructor arguments, held as std::shared_ptr<Simulation::SimulationObject6DOF>, every
member of the upper seam the two mains call -- compiled with -DAGRIFLY_USE_REFERENCE_TYPES -Werror against the tree's
Common / Components, the tree's own Onboard::QuadcopterLogic as logicType, and LINKED against the engine library plus the
tree's QuadcopterLogic.cpp / KalmanFilter6DOF.cpp objects -> oracle/_ref/dropin; and the static assertions of
tests/cpp/dropin_base_check.cpp -> oracle/_ref/dropin_base.ok.  These tests read what that left.

<Eigen/Dense> is not in the image: tests/shim/Eigen/Dense is a parse shim written for this check.  THIS IS A COMPILE AND
LINK CHECK AND PINS NOTHING: the program is never run, no number of it is compared with anything, and the oracle's
parity status (rigid-body core unpinned) is untouched by it.  Skipped where build() had no tree
to compile against (the recipe then leaves nothing under oracle/_ref/)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "oracle", "_ref")
EXE = os.path.join(OUT, "dropin")
BASE_OK = os.path.join(OUT, "dropin_base.ok")


def _read(path):
    try:
        with open(path) as f:
            return f.read()
    except OSError:
        return ""


@pytest.mark.skipif(not os.path.exists(EXE + ".log"), reason="build() compiled no drop-in check: the agri-fly tree was absent (oracle/Makefile REF)")
def test_facade_compiles_and_links_against_the_reference_headers():
    assert os.path.exists(EXE), "the drop-in build failed:\n%s\n%s" % (_read(EXE + ".facade.err")[-3000:], _read(EXE + ".log")[-3000:])
    # the façade under the reference's types: warnings are errors there, and not even a warning may remain -- a by-value /
    # const-ref or a narrowing drift is a warning first
    assert _read(EXE + ".facade.err").strip() == "", _read(EXE + ".facade.err")
    assert shutil.which("nm"), "nm is needed to read the linked program"
    # what was linked: the C ABI on one side, the reference's logicType on the other, the reference's base class in between
    syms = subprocess.run(["nm", "-C", EXE], capture_output=True, text=True, timeout=120, check=True).stdout
    for needed in ("U afe_create_host_visible", "U afe_step", "U afe_get_imu", "U afe_set_motor_cmds", "Onboard::QuadcopterLogic::Run()",
                   "agrifly::Quadcopter_T<Onboard::QuadcopterLogic>::Run()", "typeinfo for Simulation::SimulationObject6DOF"):
        assert needed in syms, needed


@pytest.mark.skipif(not os.path.exists(os.path.join(OUT, "dropin_base.log")),
                    reason="build() compiled no drop-in check: the agri-fly tree was absent (oracle/Makefile REF)")
def test_the_reference_branch_uses_the_trees_own_base_class():
    """tests/cpp/dropin_base_check.cpp: the façade's base IS the class the tree's header declares (static assertions,
    compiled -fsyntax-only -Werror by the recipe; the stamp exists only if that compile succeeded)"""
    assert os.path.exists(BASE_OK), _read(os.path.join(OUT, "dropin_base.log"))[-4000:]
    assert os.path.getmtime(BASE_OK) >= os.path.getmtime(os.path.join(ROOT, "tests", "cpp", "dropin_base_check.cpp"))


@pytest.mark.skipif(not os.path.exists(EXE + ".log"), reason="build() compiled no drop-in check: the agri-fly tree was absent (oracle/Makefile REF)")
def test_what_the_facade_derives_from_the_type_is_the_reference_constructors():
    """The one path of oracle/_ref/dropin that IS run (by the recipe, at build time; it makes no engine): for every type of
    the tree's enum, agrifly::DeriveFromType / BatteryVoltage -- what the façade's constructor uses where the caller gives
    the reference's own fifteen arguments -- equal, bit for bit, 1.2f * QuadcopterConstants(type).lowBatteryThreshold and
    the header's IMU_yaw / _pitch / _roll (Quadcopter_T.cpp:70-80), and the engine library's own table
    (afe_low_battery_threshold_from_type) equals the header's threshold.  The stamp exists only if every line agreed."""
    log = _read(os.path.join(OUT, "dropin_derive.log"))
    assert os.path.exists(os.path.join(OUT, "dropin_derive.ok")), log[-3000:]
    lines = log.splitlines()
    assert lines[-1] == "derive ok" and len(lines) == 7 and all(l.endswith(": ok") for l in lines[:6]), log[-3000:]
    assert [l.split(":")[0] for l in lines[:6]] == ["type %d" % t for t in range(6)]
    # not a stale stamp: made from the program as it is now
    assert os.path.getmtime(os.path.join(OUT, "dropin_derive.ok")) >= os.path.getmtime(EXE)
