// The device-resident halves of the two colouring entry points (coloring.hip), for the callers inside the library that keep a colouring on the
// device: label propagation (communities.hip) takes its default colouring and checks a caller's one through them, without a host round trip.
#pragma once
#include <cstdint>

#include "device_buffer.hpp"
#include "gmsx.h"

namespace gmsx {

// Jones–Plassmann under `ordering` (nullptr: the id order) with color and round_of left in the two buffers (n words each, n > 0): what
// gmsx_coloring_jp copies out.  res and *launches_out are filled; the rounds lie between the context's events ev[0] and ev[1].
int coloring_jp_device(const gmsx_graph *g, const int32_t *ordering, int rank_format, DevBuf &d_color, DevBuf &d_round, gmsx_coloring_info &res,
                       int *launches_out);
// The verifier's pass over a colouring that lies on the device: acc = the words of gmsx_coloring_verify ([0] arcs between equal colours, [1]
// colours below 1, [2] the largest colour + 2^31, [3] the largest degree, [4] distinct colours in [0, n]); ctl[1] != 0: an append hit its bound.
int coloring_verify_device(const gmsx_graph *g, const int32_t *d_color, unsigned long long acc[8], int32_t ctl[4], float *ms);

}  // namespace gmsx
