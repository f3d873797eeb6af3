// doa_pick.hpp -- the two pieces of arithmetic of bf_doa_pick_device (include/bfcore.h) that must agree bit for bit between the device,
// the host and controllers.pick_sources: the circular distance of two angles and the rule that takes an angle out of the running once
// a neighbour has been picked.  Plain C++: doa_kernels.hip includes it for the kernel, the CPU suite compiles it with g++.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define BF_PICK_HD __host__ __device__
#else
#define BF_PICK_HD
#endif

namespace bf {

// The circular distance of two angles in degrees, in [0, 180]:
//   t = (a - b) + 180,  r = fmod(t, 360),  r < 0: r += 360,  |r - 180|
// in double and in exactly this order.  The subtraction and the additions are correctly rounded and fmod is exact, so this is
// numpy's abs((a - b + 180.0) % 360.0 - 180.0) to the bit (numpy's % is fmod with the same sign fix).  A tiny negative t gives
// r + 360 = 360 after rounding and a distance of 180: kept as it is, numpy does the same.
BF_PICK_HD inline double pick_sep(double a, double b) {
    const double t = (a - b) + 180.0;
    double r = std::fmod(t, 360.0);
    if (r < 0) r += 360.0;
    return std::fabs(r - 180.0);
}

// After the angle `picked` has been taken: does the angle `a` stay free?  It leaves when its distance is below min_sep_deg (or is
// not a number: non-finite angles), as pick_sources' `free &= sep >= min_sep_deg` says.
BF_PICK_HD inline bool pick_stays_free(double a, double picked, double min_sep_deg) { return pick_sep(a, picked) >= min_sep_deg; }

}  // namespace bf
