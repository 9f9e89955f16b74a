"""scan_fov_area (csrc/scan_fov.h), the one place where the engine derives a laser scan's field-of-view area: compiled on its own with
g++ and held, bit for bit, to MeasurementModel_VictoriaPark::setLaserScan's expression (src/MeasurementModel_VictoriaPark.cpp:271-277)
restated here in the same operation order -- a running sum of neighbouring beams' products, the closing product of the first and the
last beam, then one multiplication by sin(acos(-1) / 360) / 2.  Three scans: two beams, 361 equal beams, and 361 beams of unequal
length.  The dataset extract under tests/golden/vp_extract holds no raw scans (the dataset's LASER.txt is not part of it), so the
third scan is made of the first 361 measured ranges of its measurements.dat."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

MAIN = r"""
#include <cstdio>
#include <vector>
#include "scan_fov.h"
int main() {
  int n = 0;
  if (scanf("%d", &n) != 1 || n < 2) return 1;
  std::vector<double> s(n);
  for (int k = 0; k < n; k++) if (scanf("%la", &s[k]) != 1) return 1;
  printf("%a\n", scan_fov_area(s.data(), n));
  return 0;
}
"""


def _reference(scan):
    area = 0.0
    for i in range(1, len(scan)):
        area += scan[i] * scan[i - 1]
    area += scan[0] * scan[len(scan) - 1]
    area *= math.sin(math.acos(-1) / 360) / 2
    return area


def _scans():
    meas = np.loadtxt(os.path.join(ROOT, "tests", "golden", "vp_extract", "measurements.dat"))
    ranges = meas[:361, 1]
    assert ranges.shape == (361,) and (ranges > 0).all() and np.ptp(ranges) > 1.0
    return {"two beams": np.array([12.5, 0.3]), "constant": np.full(361, 70.0), "extract": ranges}


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("scan_fov")
    src, exe = d / "main.cpp", d / "scan_fov_area"
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "rfs-slam_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("name", ["two beams", "constant", "extract"])
def test_the_area_has_the_references_bits(prog, name):
    scan = [float(v) for v in _scans()[name]]
    text = "%d\n%s\n" % (len(scan), "\n".join(v.hex() for v in scan))
    got = float.fromhex(subprocess.run([prog], input=text, capture_output=True, text=True, check=True).stdout.strip())
    want = _reference(scan)
    assert want > 0 and struct.pack("<d", got) == struct.pack("<d", want), (name, got.hex(), want.hex())


def test_the_engine_divides_by_the_area_in_one_function_only():
    src = open(os.path.join(ROOT, "rfs-slam_amd", "csrc", "rfsgpu_engine.hip")).read()
    assert "scan_fov.h" in src
    assert "sin(acos(-1) / 360)" not in src, "a second copy of the area rule"
    first, last = src.index("expectedClutterNumber / area"), src.rindex("expectedClutterNumber / area")
    assert "\n}" not in src[first:last], "the clutter density is derived in more than one function"
