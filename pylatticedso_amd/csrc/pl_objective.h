// The objective of the response sensitivities and dJ/dy: the one host look of pl_transient_sens (real outputs) and of
// pl_harmonic_sens (complex outputs).  No HIP and nothing of the handle: tests/native/objective_cases.cpp builds it with g++.
// Kind 2 is scaled by the largest |y|, so |y|^p cannot overflow.  NOT one formula: the two derivatives round differently.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>

// y[rows] real: returns J, c[n] = dJ/dy_n
inline double objective_real(int rows, const double *y, int kind, double p, const double *weight, double *c) {
  double J = 0.0;
  auto wt = [&](int n) { return weight ? weight[n] : 1.0; };
  std::fill(c, c + rows, 0.0);
  if (kind == 0) {
    for (int n = 0; n < rows; ++n) { J += wt(n) * y[n]; c[n] = wt(n); }
  } else if (kind == 1) {
    for (int n = 0; n < rows; ++n) { J += wt(n) * y[n] * y[n]; c[n] = wt(n) * y[n]; }
    J *= 0.5;
  } else {
    double top = 0.0, sum = 0.0;
    for (int n = 0; n < rows; ++n) top = std::max(top, std::fabs(y[n]));
    if (top > 0.0)
      for (int n = 0; n < rows; ++n) sum += wt(n) * std::pow(std::fabs(y[n]) / top, p);
    const double Js = sum > 0.0 ? std::pow(sum, 1.0 / p) : 0.0;
    J = top * Js;
    if (Js > 0.0)
      for (int n = 0; n < rows; ++n) {
        const double sgn = y[n] > 0.0 ? 1.0 : (y[n] < 0.0 ? -1.0 : 0.0);
        c[n] = std::pow(Js, 1.0 - p) * wt(n) * std::pow(std::fabs(y[n]) / top, p - 1.0) * sgn;
      }
  }
  return J;
}

// y[n_freq] complex, interleaved: returns J (real), g[k] = dJ/dy_k interleaved, so that dJ = sum_k Re(g_k dy_k)
inline double objective_complex(int n_freq, const double *y, int kind, double p, const double *weight, double *g) {
  double J = 0.0;
  auto wt = [&](int k) { return weight ? weight[k] : 1.0; };
  auto mag = [&](int k) { return std::hypot(y[(size_t)2 * k], y[(size_t)2 * k + 1]); };
  std::fill(g, g + (size_t)2 * n_freq, 0.0);
  if (kind == 0) {          // J = -sum w Im y, g = i w
    for (int k = 0; k < n_freq; ++k) { J -= wt(k) * y[(size_t)2 * k + 1]; g[(size_t)2 * k + 1] = wt(k); }
  } else if (kind == 1) {   // J = 1/2 sum w |y|^2, g = w conj(y)
    for (int k = 0; k < n_freq; ++k) {
      const double re = y[(size_t)2 * k], im = y[(size_t)2 * k + 1];
      J += wt(k) * (re * re + im * im);
      g[(size_t)2 * k] = wt(k) * re;
      g[(size_t)2 * k + 1] = -wt(k) * im;
    }
    J *= 0.5;
  } else {
    double top = 0.0, sum = 0.0;
    for (int k = 0; k < n_freq; ++k) top = std::max(top, mag(k));
    if (top > 0.0)
      for (int k = 0; k < n_freq; ++k) sum += wt(k) * std::pow(mag(k) / top, p);
    const double Js = sum > 0.0 ? std::pow(sum, 1.0 / p) : 0.0;
    J = top * Js;
    if (Js > 0.0)
      for (int k = 0; k < n_freq; ++k) {
        const double a = mag(k) / top;
        const double c = a > 0.0 ? std::pow(Js, 1.0 - p) * wt(k) * std::pow(a, p - 2.0) / top : 0.0;
        g[(size_t)2 * k] = c * y[(size_t)2 * k];
        g[(size_t)2 * k + 1] = -c * y[(size_t)2 * k + 1];
      }
  }
  return J;
}
