// halo_segs.h -- the segment cap of one halo exchange (restir_halo_plan): HaloSegs (restir_types.h) and the plain C++
// layout unit (layout.cpp, through layout.h) size their arrays by it.
#pragma once

#define RESTIR_MAX_HALO_SEGS 8u
