// abi_error.cpp -- the one thread-local error string behind restir_last_error, and fail() that sets it (abi_error.h).
#include "abi_error.h"

#include <cstdarg>
#include <cstdio>
#include <string>

namespace {
thread_local std::string g_err;
}  // namespace

extern "C" const char* restir_last_error(void) { return g_err.c_str(); }

namespace romis {

restir_status fail(restir_status s, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return s;
}

}  // namespace romis
