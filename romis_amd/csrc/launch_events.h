// launch_events.h -- host side shared by the launchers of kernels.hip and mis.hip: the timed-launch event pair and the
// launch shape constants (launch_shape.h).
#pragma once

#include <hip/hip_ext.h>

#include "launch_shape.h"

namespace romis {

// Timed launches: restir.cpp's TIMED hands a start / stop event pair to the next launch, which records them inside its
// own dispatch (hipExtLaunchKernelGGL) -- no separate event packets, hence no stream gaps.
inline thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;
inline thread_local bool g_launched = false;

#define ROMIS_LAUNCH(kernel, grid, block, lds, stream, ...)                                                    \
    do {                                                                                                      \
        /* a multi-launch stage: start event on its first kernel, stop event after its last */              \
        hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, g_launched ? nullptr : g_ev_start, g_ev_stop, 0, \
                              __VA_ARGS__);                                                                   \
        g_launched = true;                                                                                    \
    } while (0)

}  // namespace romis
