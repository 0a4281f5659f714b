// abi_error.h -- the C ABI's error reporting, for every unit behind include/restir_c.h.  No HIP header: layout.cpp and
// abi_error.cpp compile as plain C++ (like bvh.cpp).
#pragma once

#include "restir_c.h"

namespace romis {

// Sets the calling thread's restir_last_error text (abi_error.cpp holds the one string) and returns s.
restir_status fail(restir_status s, const char* fmt, ...);

}  // namespace romis

#define ST_TRY(expr)                            \
    do {                                        \
        restir_status s_ = (expr);              \
        if (s_ != RESTIR_OK) return s_;         \
    } while (0)
