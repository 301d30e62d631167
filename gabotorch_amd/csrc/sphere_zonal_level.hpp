// One level of a zonal series on the sphere (csrc/sphere_zonal.hip states the series and its recurrence): the coefficient of P_k and the factor
// B_k = (k - 1) / (k + d - 2) of  P_k = t + B_k (t - P_{k-2}),  t = c P_{k-1}  (series dimension d; B_0 = B_1 = 0).  Shared by the Gram / element-wise
// kernels of sphere_zonal.hip, which take a series by value, and the acquisition kernels of sphere_tr.hip, which read a table of them from memory.
#pragma once

namespace gabo {

constexpr int kZonalMaxCoeff = 129;

struct ZonalLevel {
    double a, rb;          // coeff_k, B_k
};

}  // namespace gabo
