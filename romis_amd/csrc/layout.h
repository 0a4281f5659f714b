// layout.h -- what layout.cpp (tile layouts and halo plans, plain C++) shares with the other units behind
// include/restir_c.h.  No HIP header.
#pragma once

#include "halo_segs.h"
#include "restir_c.h"

namespace romis {

// a layout's cuts are well formed: every column and every row of a column at least one pixel, the ends at the image
restir_status layout_check(const restir_tile_layout* L);
// The operations restir_halo_pass posts, from a plan: send i then recv i per segment (restir_halo_ops)
void halo_ops_from(const restir_halo_segment* send, const restir_halo_segment* recv, uint32_t n, restir_halo_op* ops);

}  // namespace romis
