// Shared by the labelled ground-truth enumerators (groundtruth_label.cpp, groundtruth_label_dev.hip).
#pragma once
#include <stdint.h>

namespace desco {

constexpr int GTL_KMAX_DEV = 5;      // largest query of the device path
constexpr int GTL_AMAX_DEV = 16;     // label ids of the device path: 4 bits
constexpr int GTL_KMAX_HOST = 6;
constexpr int GTL_AMAX_HOST = 256;   // label ids of the host path: 8 bits (6 of them + 15 mask bits in one 64-bit code)

// The device's lookup table.  A found subset of k nodes with induced adjacency mask m (bit b(b-1)/2 + a
// for the pair a < b of subset positions) and label ids l_0..l_{k-1} (subset order) reads entry
//   off[k] + m * A^k + sum_j l_j * A^j
// where the blocks of k = 2, 3, .. follow each other: off[2] = 0, off[k+1] = off[k] + 2^(k(k-1)/2) * A^k.
struct GtlLayout {
  int64_t off[GTL_KMAX_DEV + 2];     // off[kmax + 1] = number of entries
  int64_t apow[GTL_KMAX_DEV + 1];    // A^j
};

inline GtlLayout gtl_layout(int kmax, int num_labels) {
  GtlLayout l{};
  l.apow[0] = 1;
  for (int j = 1; j <= GTL_KMAX_DEV; ++j) l.apow[j] = l.apow[j - 1] * num_labels;
  for (int k = 2; k <= GTL_KMAX_DEV; ++k)
    l.off[k + 1] = l.off[k] + (k <= kmax ? ((int64_t)1 << (k * (k - 1) / 2)) * l.apow[k] : 0);
  return l;
}

}  // namespace desco
