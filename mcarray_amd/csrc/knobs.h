// knobs.h -- the only place of the library that looks at the environment.
// Product switches are read ONCE per context, at creation (api.hip: read_knobs).
#pragma once
#include <cstdlib>

namespace mca {

inline const char *env_str(const char *name) { return std::getenv(name); }

}  // namespace mca
