"""tests/golden/physics_ref.npz, made by the reference itself (run: python tests/golden/make_golden_physics.py).

TEST INFRASTRUCTURE.  The scenarios of tests/oracle_phys.py (SCENARIOS) are run through the
reference's own Additive<double> / Minimizer<double>::physics(): ref_physics_driver.cpp (next to this
file) is compiled into oracle/_ref/ with the REF_CXXFLAGS and the stub headers of oracle/Makefile, and
the npz holds, per scenario, the audio and the particle positions after every physics step.  Data
only.  Without the reference's sources the script prints one line and leaves the fixture as it is.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from oracle_phys import SCENARIOS  # noqa: E402

ORACLE = os.path.join(ROOT, "oracle")
BIN = os.path.join(ORACLE, "_ref", "ref_physics_driver")


def makefile_var(name):
    txt = open(os.path.join(ORACLE, "Makefile")).read()
    return re.search(rf"^{name} \?= (.*)$", txt, re.M).group(1).strip()


def build():
    ref_src = os.environ.get("REF_SRC") or makefile_var("REF_SRC")
    if not os.path.exists(os.path.join(ref_src, "minimizer.h")):
        return False
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, *makefile_var("REF_CXXFLAGS").split(), "-iquote", ref_src,
                    "-I" + os.path.join(ORACLE, "ref", "stubs"), "-o", BIN,
                    os.path.join(HERE, "ref_physics_driver.cpp")], check=True)
    return True


def reference(sc):
    P = sc["V"] * sc["O"]
    lines = [f"{sc['V']} {sc['O']} {float(sc['decay']).hex()} {float(sc['harm']).hex()} {float(sc['k']).hex()} "
             f"{sc['period']}"]
    pos = 0
    for t in sorted({t for t, *_ in sc["events"]} | {sc["n"]}):
        if t > pos:
            lines.append(f"run {t - pos}")
            pos = t
        for et, kind, a, b in sc["events"]:
            if et == t and t < sc["n"]:
                lines.append(f"ev {kind} {float(a).hex()} {float(b).hex()}")
    lines.append("end")
    with tempfile.TemporaryDirectory() as d:
        case, out = os.path.join(d, "case.txt"), os.path.join(d, "out.f64")
        with open(case, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.run([BIN, case, out], check=True, timeout=120)
        y = np.fromfile(out, dtype="<f8")
    return y[:sc["n"]].copy(), y[sc["n"]:].reshape(-1, P).copy()


def main():
    if not build():
        print("make_golden_physics: no reference sources; tests/golden/physics_ref.npz left as it is")
        return
    d = {"made_by": "reference"}
    for name, sc in SCENARIOS.items():
        d[name + "_audio"], d[name + "_track"] = reference(sc)
        print(name, d[name + "_track"].shape)
    np.savez(os.path.join(HERE, "physics_ref.npz"), **d)


if __name__ == "__main__":
    main()
