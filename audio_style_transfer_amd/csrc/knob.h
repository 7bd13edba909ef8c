// The one reader of the ASTYLE_* tuning knobs (host only, no HIP includes; common.h includes it).
// A call site keeps the value in a function-local static,
//     static const int nc = env_int("ASTYLE_...", 0, {4, 8});
// so the environment is read once per process, at the first use, and a knob cannot change between
// two launches.  A value outside the knob's stated domain is the default, as if the variable were
// unset.  What a knob is for, and what was measured with it, is said at its call site.
#pragma once
#include <stdlib.h>
#include <limits.h>
#include <initializer_list>

namespace ast {

// the integer value of `name` if it lies in [lo, hi], else (or unset) `def`
inline long env_int(const char* name, long def, long lo = LONG_MIN, long hi = LONG_MAX) {
    const char* e = getenv(name);
    if (!e) return def;
    const long v = strtol(e, nullptr, 10);
    return v < lo || v > hi ? def : v;
}
// the integer value of `name` if it is one of `allowed`, else (or unset) `def`
inline long env_int(const char* name, long def, std::initializer_list<long> allowed) {
    const long v = env_int(name, def);
    for (long a : allowed) if (v == a) return v;
    return def;
}
// a switch: `def` while unset (any value, e.g. -1 for "not forced"), else 1 for non-zero and 0 for zero
inline int env_flag(const char* name, int def) {
    const char* e = getenv(name);
    return e ? (strtol(e, nullptr, 10) != 0 ? 1 : 0) : def;
}

}  // namespace ast
