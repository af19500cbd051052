// Node words of the PCG vector kernels (pl_coarse.h): one 4-byte word per node, {rx, ry, rz, class}.
//   bytes 0-2  the node's lever arm to its aggregate's reference point as three signed bytes in units of 2^-e
//   byte  3    the class of the node's Jacobi weights (rebuilt on the device at every assembly: k_dcl_* in pl_coarse.h)
// This header is the HOST side of the lever arms: the search for e and the packing.  No HIP include, so that it compiles
// and is tested without a GPU (tests/native/nodeword_main.cpp).
//
// The bytes are used only where (double)int8 * 2^-e gives the lever arm back BIT FOR BIT, node by node - a condition, not a
// tolerance: the coarse modes must stay exactly rigid per aggregate (see Coarse::rel32).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pl {

constexpr int kRelByteMaxExp = 8;     // e in 0 .. 8: units of 1, 1/2, ... 1/256
constexpr int kRelByteMaxMag = 127;   // symmetric range of a signed byte (-128 is left out)

inline bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// Smallest e in 0 .. kRelByteMaxExp for which every d[i] * 2^e is an integer of magnitude <= 127; -1 if there is none
// (not dyadic, finer than 2^-8, or too long).  Scaling by a power of two is exact, so the test is too.
inline int rel_byte_exponent(const double *d, size_t n) {
  int e = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!std::isfinite(d[i])) return -1;
    for (;;) {
      const double s = std::ldexp(d[i], e);
      if (std::fabs(s) > (double)kRelByteMaxMag) return -1;   // a larger e only makes it longer
      if (s == std::floor(s)) break;
      if (++e > kRelByteMaxExp) return -1;
    }
  }
  for (size_t i = 0; i < n; ++i)                                // entries accepted before e grew
    if (std::fabs(std::ldexp(d[i], e)) > (double)kRelByteMaxMag) return -1;
  return e;
}

// The lever arm a kernel reconstructs from byte b (the same expression as on the device: an exact product)
inline double rel_byte_value(int8_t b, int e) { return (double)b * std::ldexp(1.0, -e); }
inline int8_t node_word_byte(uint32_t w, int k) { return (int8_t)(uint8_t)(w >> (8 * k)); }

// d = [3 n_nodes] lever arms.  On success: words[i] = {rx, ry, rz, 0} and e; returns false (words untouched) where the
// bytes cannot carry every lever arm exactly - which includes a -0.0, whose sign a byte cannot hold.
inline bool pack_rel_bytes(const double *d, size_t n_nodes, std::vector<uint32_t> &words, int &e_out) {
  const int e = rel_byte_exponent(d, 3 * n_nodes);
  if (e < 0) return false;
  std::vector<uint32_t> w(n_nodes);
  for (size_t i = 0; i < n_nodes; ++i) {
    uint32_t word = 0;
    for (int k = 0; k < 3; ++k) {
      const int8_t b = (int8_t)(int)std::ldexp(d[3 * i + k], e);
      if (!same_bits(rel_byte_value(b, e), d[3 * i + k])) return false;
      word |= (uint32_t)(uint8_t)b << (8 * k);
    }
    w[i] = word;
  }
  words.swap(w);
  e_out = e;
  return true;
}

}  // namespace pl
