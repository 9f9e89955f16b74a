// The field-of-view area of a laser scan, as MeasurementModel_VictoriaPark::setLaserScan sums it
// (src/MeasurementModel_VictoriaPark.cpp:271-277): the products of neighbouring beams, the last with the first, times sin(pi / 360) / 2.
// A filter's clutter density is its expectedClutterNumber over this area, and the density's bits feed every Victoria Park parity
// test, so the operations and their order are the reference's.  Plain C++: tests/test_scan_fov_area.py compiles it without HIP.
#pragma once
#include <cmath>

static inline double scan_fov_area(const double *scan, int n) {
  double area = 0;
  for (int k = 1; k < n; k++) area += scan[k] * scan[k - 1];
  area += scan[0] * scan[n - 1];
  area *= sin(acos(-1) / 360) / 2;
  return area;
}
