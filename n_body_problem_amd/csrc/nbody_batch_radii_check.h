// nbody_batch_radii_check.h -- what nbody_batch_radii_set (include/nbody_batch_radii.h) accepts, free of HIP so that a CPU
// test can compile it: one radius per slot, finite and >= 0 in every slot below its system's count.  Slots beyond the count
// are not examined.
#ifndef NBODY_AMD_BATCH_RADII_CHECK_H
#define NBODY_AMD_BATCH_RADII_CHECK_H

#include <cmath>
#include <cstdint>
#include <string>

namespace nbody {

// radii: n_systems x max_bodies, system s at s * max_bodies; counts: n_systems.  false, and in *msg the first system and
// slot refused, when a radius below the count is negative or not finite.
inline bool batch_radii_ok(const float *radii, const int *counts, int64_t n_systems, int64_t max_bodies, std::string *msg)
{
    for (int64_t s = 0; s < n_systems; ++s)
        for (int64_t i = 0; i < counts[s] && i < max_bodies; ++i) {
            const float r = radii[s * max_bodies + i];
            if (!std::isfinite(r) || r < 0.f) {
                if (msg)
                    *msg = "radius of system " + std::to_string(s) + ", slot " + std::to_string(i) + " (" + std::to_string(r) +
                           ") must be finite and >= 0";
                return false;
            }
        }
    return true;
}

}  // namespace nbody

#endif  // NBODY_AMD_BATCH_RADII_CHECK_H
