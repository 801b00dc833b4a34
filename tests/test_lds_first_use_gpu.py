"""GPU: every kernel that launches with more dynamic LDS than the default limit gets its limit
raised by the object that launches it (hz::allow_lds, huygens_amd/csrc/hz_lds.h), not by whatever
object the process happened to create before.  Each case is a fresh Python process whose first
library object is the one under test (tests/lds_first_use_cases.py), so no other engine's create
can have raised a limit on its behalf: Cosine(8192) used to rely on an STFT handle having been
created first.  Inputs, references and bounds are those of the tests that already cover each object."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# case -> (comparisons printed, bound)
CASES = {
    "cosine": (2, 1e-13),    # test_stft_spectrum_gpu.py::test_cosine_every_size
    "stft_p4": (1, 1e-10),   # test_stft_spectrum_gpu.py TOL
    "freezer": (1, 1e-9),    # test_freezer_gpu.py TOL
    "bowl": (2, 1e-9),       # test_bowl_gpu.py, T = double
}


@pytest.mark.parametrize("case", list(CASES))
def test_first_object_in_a_fresh_process(gpu_lib, case):
    count, bound = CASES[case]
    r = subprocess.run([sys.executable, os.path.join(HERE, "lds_first_use_cases.py"), case], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    errs = [float(m) for m in re.findall(r"^err (\S+)$", r.stdout, re.M)]
    print(case, errs)
    assert len(errs) == count, r.stdout
    assert all(e < bound for e in errs), errs   # (a NaN fails)
